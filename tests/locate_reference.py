"""Numpy restatement of the field tape's grid-search hypocentre location (the device side is loc_search_kernel and
loc_finish_kernel of ttcr_amd/csrc/fsm_locate.hip) and a stand-in tape built from given fields, with which inversion.locate runs
without a device.  Everything is float64, every difference, product, quotient and sum rounded on its own (numpy does not fuse), the
sums from +0 in ascending pick order: a loop over the picks of a hypocentre, vectorised over the nodes.

Conventions as in adjoint_reference: node m = (k * nny + j) * nnx + i (x fastest); nn3 = (nnx, nny, nnz).  csr = (off, field, time,
weight): the picks of hypocentre q are off[q] .. off[q + 1], weight may be None (all ones).  box = ((i0, i1), (j0, j1), (k0, k1)),
half-open node ranges, or None for the whole grid; box nodes are numbered x fastest within the box.
"""
import numpy as np

import receiver_reference as RR


def csr_of(pick_hypo, pick_field, pick_time, pick_weight=None, n_hypo=None):
    """the picks grouped by hypocentre in ascending pick index (a stable grouping): (off, field, time, weight)"""
    hyp = np.asarray(pick_hypo, dtype=np.int64)
    n_hypo = (int(hyp.max()) + 1 if hyp.size else 0) if n_hypo is None else int(n_hypo)
    order = np.argsort(hyp, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(hyp, minlength=n_hypo))]).astype(np.int64)
    wt = None if pick_weight is None else np.asarray(pick_weight, dtype=np.float64)[order]
    return off, np.asarray(pick_field, dtype=np.int64)[order], np.asarray(pick_time, dtype=np.float64)[order], wt


def box_nodes(nn3, box):
    """node index (of the whole grid) of every box node, in the box's own numbering (x fastest within the box)"""
    box = tuple((0, n) for n in nn3) if box is None else box
    (i0, i1), (j0, j1), (k0, k1) = box
    k, j, i = np.meshgrid(np.arange(k0, k1), np.arange(j0, j1), np.arange(i0, i1), indexing="ij")
    return ((k * nn3[1] + j) * nn3[0] + i).ravel().astype(np.int64)


def misfit(values, time, weight):
    """(sw, t0, phi) of one hypocentre: values (K, n) = the field value of every pick at n places, float64"""
    K, n = values.shape
    sw = np.float64(0.0)
    for k in range(K):
        sw = sw + weight[k]
    a = np.zeros(n)
    for k in range(K):
        a = a + weight[k] * (time[k] - values[k])
    with np.errstate(invalid="ignore", divide="ignore"):
        t0 = a / sw
    phi = np.zeros(n)
    for k in range(K):
        d = (time[k] - values[k]) - t0
        phi = phi + weight[k] * (d * d)
    return sw, t0, phi


def grid_search(T, nn3, csr, box=None):
    """(node, t0, misfit, volume): T (n_fields, n_nodes) fields of any float dtype; node (n_hypo,) int64 -- the box node with the smallest
    phi, the lowest index among equal ones, a NaN never winning, -1 if sw == 0 or every phi is NaN --, t0 and misfit there (+0 for -1),
    volume (n_hypo, nk, nj, ni) = phi of every box node (+0 rows for sw == 0)"""
    off, field, time, weight = csr
    T = np.asarray(T)
    T = T.reshape(T.shape[0], -1)
    nodes = box_nodes(nn3, box)
    box = tuple((0, n) for n in nn3) if box is None else box
    shape = tuple(b[1] - b[0] for b in reversed(box))
    nq = len(off) - 1
    node, t0, mis = np.full(nq, -1, dtype=np.int64), np.zeros(nq), np.zeros(nq)
    vol = np.zeros((nq,) + shape)
    for q in range(nq):
        ks = slice(off[q], off[q + 1])
        w = np.ones(off[q + 1] - off[q]) if weight is None else weight[ks]
        vals = T[field[ks]][:, nodes].astype(np.float64)          # (exact for an fp32 field)
        sw, t0n, phi = misfit(vals, time[ks], w)
        if sw == 0:
            continue
        vol[q] = phi.reshape(shape)
        if np.all(np.isnan(phi)):
            continue
        b = int(np.nanargmin(phi))                                 # (the first of the smallest: the lowest node index)
        node[q], t0[q], mis[q] = nodes[b], t0n[b], phi[b]
    return node, t0, mis, vol


class StandInTape:
    """What inversion.locate needs of a FieldTape, from given fields (n_fields arrays of n_nodes values in the grid dtype) on the host:
    geometry, n_events, locate_grid (the restatement above), receiver_eval (receiver_reference.evaluate on the points as the solver sees
    them: rounded to the fields' dtype, the origin of a translated grid subtracted in that dtype) and node_coordinates."""

    def __init__(self, fields, nn3, dx, origin=(0.0, 0.0, 0.0), translate=False):
        self.fields = [np.asarray(f).ravel() for f in fields]
        self.dtype = self.fields[0].dtype
        self.nn3, self.dx, self.origin, self.translate = tuple(int(n) for n in nn3), float(dx), np.asarray(origin, dtype=np.float64), translate
        self.n_events = len(self.fields)
        self.n_nodes = int(np.prod(self.nn3))
        self.evals = 0   # receiver_eval calls

    @property
    def geometry(self):
        return self.nn3, self.dx, self.origin.copy()

    def locate_grid(self, pick_hypo, pick_field, pick_time, pick_weight=None, n_hypo=None, box=None, return_misfit=False):
        out = grid_search(np.stack(self.fields), self.nn3, csr_of(pick_hypo, pick_field, pick_time, pick_weight, n_hypo), box)
        return out if return_misfit else out[:3]

    def receiver_eval(self, pts, event_of_pt, return_grad=True):
        dt = self.dtype
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3).astype(dt)
        self.evals += 1
        if self.translate:
            pts, mn = (pts - self.origin.astype(dt)).astype(dt), (0.0, 0.0, 0.0)
        else:
            mn = tuple(self.origin)
        tt, G = RR.evaluate_points(self.fields, self.nn3, self.dx, mn, pts, np.asarray(event_of_pt))
        return (tt, G) if return_grad else tt

    def node_coordinates(self, node):
        node = np.asarray(node, dtype=np.int64).reshape(-1)
        nx, ny = self.nn3[0], self.nn3[1]
        ijk = np.stack([node % nx, (node // nx) % ny, node // (nx * ny)], axis=1)
        xyz = self.origin[None, :] + ijk.astype(np.float64) * self.dx
        xyz[node < 0] = np.nan
        return xyz
