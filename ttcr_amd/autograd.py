"""ttcr_amd.autograd -- traveltimes as a differentiable torch operator (no ttcrpy counterpart).

    tt = ttcr_amd.autograd.raytrace(grid, velocity, source, rcv, aggregate_src=False)

`grid` is a 3-D node grid (Grid3d(..., cell_slowness=0)); `velocity` a torch tensor of node velocities, shape (nx, ny, nz) or flat in
C order (what Grid3d.set_velocity reads).  The forward sets the model as set_velocity does (through the host: 1 / velocity in numpy,
then the grid dtype) and runs grid.raytrace_tape; tt is a tensor of the grid dtype on velocity's device, bit-equal to
raytrace(..., compute_M=True)[0].  The backward is M^T g (MTape.vjp, on the device) permuted to velocity's layout, where M is the
reference's matrix of d tt / d velocity with the rays held fixed: the gradient of the ray-frozen (linearised) problem, not the exact
derivative of the returned tt.  A model in slowness composes in torch: raytrace(grid, 1 / s, ...).  A second derivative through this
operator raises (its backward is marked once_differentiable).

    tt = ttcr_amd.autograd.raytrace_adjoint(grid, velocity, source, rcv, aggregate_src=False, return_fields=False)

is the same operator with the EXACT derivative: the forward runs grid.raytrace_adjoint (interpolated receiver traveltimes, as a grid
with tt_from_rp=0 returns them; 3-D node grids with weno=0), the backward is the adjoint-state gradient FieldTape.vjp -- the derivative
of the returned tt through the solver's own first-order update -- times d slowness / d velocity = -1 / velocity**2, in velocity's layout.
With return_fields=True it returns (tt, fields), fields the (n_events, nx, ny, nz) traveltime fields, differentiable too: a loss on the
grid traveltimes has a gradient.  The backward is itself differentiable (create_graph=True, torch.autograd.functional.hvp, gradient
penalties): the second derivative with respect to velocity is exact -- FieldTape.jvp for the part through the cotangent, FieldTape.hvp
(the second-order term of the solver's own linearisation) for the part through the model, and the derivative of the factor
-1 / velocity**2 --, on node and cell grids, with and without return_fields.  The double backward is linear in its own cotangent
and differentiable in it (torch.autograd.functional.hvp's double-backward trick works); a third derivative raises.  Forward mode works as well (torch.autograd.forward_ad): the tangent of the outputs for a velocity
tangent tv is FieldTape.jvp(-(tv / velocity**2)), J v of the same linearisation, in the layout of the outputs.

    tt = ttcr_amd.autograd.raytrace_events(grid, velocity, events, event_of_row, rcv, return_fields=False)

is raytrace_adjoint for events that are themselves unknowns: `events` is an (n_events, 4) tensor of (t0, x, y, z), one source point
per event, `event_of_row` names the event of every rcv row (every event needs a row), and the operator is differentiable with respect
to velocity AND events.  The backward is one FieldTape.vjp(..., return_source_grad=True): the slowness gradient as above and the exact
derivative with respect to the origin time and the position of every event, through the nodes the source initialisation froze.  Forward
mode adds FieldTape.jvp and FieldTape.jvp_source.  The derivative with respect to a position has a kink where the point crosses a cell
face or comes within 1e-4 of a node: the formula of the side the point is on is returned.  Second derivatives through raytrace_events
(with respect to the source points, and mixed ones) are not implemented: a double backward raises instead of returning a part.

raytrace_adjoint and raytrace_events are differentiable in `rcv` too when it is a torch tensor that requires grad (or carries a forward
tangent): the backward is g[r] * G[r], G = FieldTape.receiver_jacobian() -- the derivative of the receiver interpolation as the solver
evaluates it --, forward mode adds FieldTape.jvp_receiver's rows.  A second derivative through rcv raises.

Both take wrt='nodes' (default) or wrt='cells'.  With wrt='cells' `grid` is a 3-D cell grid (Grid3d(..., cell_slowness=1, weno=0)),
`velocity` holds one value per cell, shape (ncx, ncy, ncz) or flat in C order, and the derivative is the one with respect to the cell
velocities (FieldTape of raytrace_adjoint(..., wrt='cells'): the node tape composed with the cell-to-node averaging of set_slowness);
fields and their cotangents stay (n_events, nx, ny, nz) node arrays.

    s = ttcr_amd.autograd.prolong(grid, m, model_shape)          g_m = ttcr_amd.autograd.restrict(grid, g, model_shape)

are the trilinear prolongation P from a coarse model grid onto the grid's nodes and its transpose (Grid3d.prolong / Grid3d.restrict,
DESIGN.md 6n) as torch operators: m holds (mx, my, mz) values (or flat in C order), s is (nx, ny, nz); the backward of each is the other,
and because both are linear, forward mode and double backward follow.  raytrace_adjoint(grid, 1 / prolong(grid, m, shape), source, rcv)
is then differentiable in the coarse slowness m; the existing operators need no new keyword.

torch is imported when this module is used, never by `import ttcr_amd`.
"""
import numpy as np

_Fn = None
_AdjFn = None
_EvFn = None
_MapFns = None


def _function():
    global _Fn
    if _Fn is not None:
        return _Fn
    import torch
    from torch.autograd.function import once_differentiable

    class RaytraceFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, velocity, grid, source, rcv, aggregate_src):
            grid.set_velocity(velocity.detach().cpu().numpy())
            tt, tape = grid.raytrace_tape(source, rcv, aggregate_src=aggregate_src)
            ctx.tape = tape
            ctx.layout = (tuple(velocity.shape), velocity.dtype, (grid.x.size, grid.y.size, grid.z.size))
            return torch.from_numpy(tt).to(velocity.device)

        @staticmethod
        @once_differentiable   # (M is the ray-frozen matrix: a second derivative through it would be a partial one)
        def backward(ctx, g):
            shape, vdt, (nx, ny, nz) = ctx.layout
            gn = ctx.tape.vjp(g.contiguous())
            # node order x fastest -> (nx, ny, nz) in C order -> velocity's layout
            gv = gn.reshape(nz, ny, nx).permute(2, 1, 0).contiguous().reshape(shape)
            return gv.to(vdt), None, None, None, None

    _Fn = RaytraceFn
    return _Fn


def raytrace(grid, velocity, source, rcv, aggregate_src=False):
    """Traveltimes at `rcv` for the model `velocity` (torch tensor, node grid layout); differentiable with respect to velocity
    (backward = M^T g, M the ray-frozen derivative of compute_M).  See the module docstring."""
    if grid._ndim != 3:
        raise NotImplementedError('compute_M is implemented for 3-D grids only')
    if grid.cell_slowness:
        raise NotImplementedError('compute_M not defined for grids with slowness defined for cells')
    source = np.asarray(source)
    rcv = np.asarray(rcv)
    return _function().apply(velocity, grid, source, rcv, bool(aggregate_src))


def _adjoint_function():
    global _AdjFn
    if _AdjFn is not None:
        return _AdjFn
    import torch
    from torch.autograd.function import once_differentiable

    def to_model(a, layout):
        """velocity's layout -> (mx, my, mz) in C order -> model order x fastest"""
        (mx, my, mz) = layout[2]
        return a.reshape(mx, my, mz).permute(2, 1, 0).contiguous().reshape(-1)

    def from_model(a, layout):
        """model order x fastest -> (mx, my, mz) in C order -> velocity's layout"""
        (mx, my, mz) = layout[2]
        return a.reshape(mz, my, mx).permute(2, 1, 0).contiguous().reshape(layout[0])

    def field_cot(gf):
        """(n_events, nx, ny, nz) in C order -> node order x fastest"""
        return None if gf is None else gf.permute(0, 3, 2, 1).contiguous().reshape(gf.shape[0], -1)

    def fields_out(df, layout):
        """(n_events, n_nodes) node order x fastest -> (n_events, nx, ny, nz) in C order"""
        nx, ny, nz = layout[1]
        return df.reshape(df.shape[0], nz, ny, nx).permute(0, 3, 2, 1).contiguous()

    class _NoThirdFn(torch.autograd.Function):
        """identity whose backward raises: put on the inputs the second derivative depends on beyond what is implemented, so that a
        third derivative raises where autograd would otherwise return a part of it"""

        @staticmethod
        def forward(ctx, a):
            return a.view_as(a)

        @staticmethod
        def backward(ctx, c):
            raise RuntimeError('raytrace_adjoint is differentiable twice: third derivatives are not implemented')

    def no_third(a):
        return a if a is None or not a.requires_grad else _NoThirdFn.apply(a)

    def second_order(gg, g, gf, velocity, tape, layout, need):
        """(grad_g, grad_gf, grad_v) of y = -P vjp(g, gf) / v^2 for the cotangent gg of y (P: model order -> velocity's layout):
        y is linear in (g, gf) -- the transpose is the jvp of ds = P^T(-gg / v^2) --; through the slowness its derivative is the hvp for
        the held cotangent (g, gf) between the two factors -1 / v^2, plus the derivative of the outer factor, 2 h gg / v^3, h = P vjp"""
        v2 = velocity * velocity
        ds = to_model(-(gg / v2), layout)
        grad_g = grad_gf = grad_v = None
        if need[0] or need[1]:
            if gf is not None and need[1]:
                dtt, df = tape.jvp(ds, return_fields=True)
                grad_gf = fields_out(df, layout).to(gf.dtype)
            else:
                dtt = tape.jvp(ds)
            grad_g = dtt.to(g.dtype)
        if need[2]:
            h = from_model(tape.hold(g.contiguous(), field_cot(gf), return_grad=True), layout).to(velocity.dtype)
            hv = from_model(tape.hvp(ds), layout).to(velocity.dtype)
            grad_v = -hv / v2 + 2 * h * gg / (v2 * velocity)
        return grad_g, grad_gf, grad_v

    class _AdjDoubleBackwardFn(torch.autograd.Function):
        """The double backward as a function of its cotangent gg, in which it is linear: differentiable with respect to gg (what
        torch.autograd.functional.hvp's double-backward trick needs); g, gf and velocity come in behind _NoThirdFn."""

        @staticmethod
        def forward(ctx, gg, g, gf, velocity, tape, layout, need):
            ctx.tape, ctx.layout, ctx.has_gf = tape, layout, gf is not None
            ctx.save_for_backward(g, gf, velocity)
            ctx.set_materialize_grads(False)
            outs = second_order(gg, g, gf, velocity, tape, layout, need)
            ctx.mark_non_differentiable(*[o for o, n in zip(outs, need) if o is not None and not n])
            return outs

        @staticmethod
        @once_differentiable
        def backward(ctx, c_g, c_gf, c_v):
            # the transpose of a map that is symmetric up to the layout: gg -> (J ds, H ds + ...) has the transpose
            # (c_g, c_gf, c_v) -> -P vjp(c_g, c_gf) / v^2 + second_order(c_v)[2]
            g, gf, velocity = ctx.saved_tensors
            tape, layout = ctx.tape, ctx.layout
            out = None
            if c_g is not None or c_gf is not None:
                if c_g is None:
                    c_g = torch.zeros_like(g)
                out = -from_model(tape.vjp(c_g.contiguous(), field_cot(c_gf)), layout).to(velocity.dtype) / (velocity * velocity)
            if c_v is not None:
                part = second_order(c_v, g, gf, velocity, tape, layout, (False, False, True))[2]
                out = part if out is None else out + part
            zero = lambda a: None if a is None else torch.zeros_like(a)   # noqa: E731  (behind _NoThirdFn: raises if it is ever used)
            return out, zero(g), zero(gf), zero(velocity), None, None, None

    class _AdjBackwardFn(torch.autograd.Function):
        """The backward of RaytraceAdjointFn as a function of (g, gf, velocity), differentiable once more: see second_order."""

        @staticmethod
        def forward(ctx, g, gf, velocity, tape, layout):
            ctx.tape, ctx.layout = tape, layout
            ctx.save_for_backward(g, gf, velocity)
            gn = tape.vjp(g.contiguous(), field_cot(gf))
            # d slowness / d velocity = -1 / velocity^2
            return -from_model(gn, layout).to(velocity.dtype) / (velocity * velocity)

        @staticmethod
        def backward(ctx, gg):
            g, gf, velocity = ctx.saved_tensors
            need = (ctx.needs_input_grad[0], gf is not None and ctx.needs_input_grad[1], ctx.needs_input_grad[2])
            if not torch.is_grad_enabled():
                return second_order(gg, g, gf, velocity, ctx.tape, ctx.layout, need) + (None, None)
            outs = _AdjDoubleBackwardFn.apply(gg, no_third(g), no_third(gf), no_third(velocity), ctx.tape, ctx.layout, need)
            return tuple(outs) + (None, None)

    class RaytraceAdjointFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, velocity, grid, source, rcv, aggregate_src, return_fields, wrt, holder):
            grid.set_velocity(velocity.detach().cpu().numpy())
            tt, tape = grid.raytrace_adjoint(source, rcv, aggregate_src=aggregate_src, wrt=wrt)
            holder.append(tape)   # (for the receiver term: _with_receiver_term)
            nx, ny, nz = grid.x.size, grid.y.size, grid.z.size
            ctx.tape = tape
            ctx.layout = (tuple(velocity.shape), (nx, ny, nz), _model_dims(grid, wrt))
            ctx.save_for_backward(velocity)
            ctx.save_for_forward(velocity)
            ctx.return_fields = return_fields
            out = torch.from_numpy(tt).to(velocity.device)
            if not return_fields:
                return out
            f = np.stack([tape.field(e).reshape(nz, ny, nx).transpose(2, 1, 0) for e in range(tape.n_events)])
            return out, torch.from_numpy(np.ascontiguousarray(f)).to(velocity.device)

        @staticmethod
        def backward(ctx, g, gf=None):
            (velocity,) = ctx.saved_tensors
            return _AdjBackwardFn.apply(g, gf, velocity, ctx.tape, ctx.layout), None, None, None, None, None, None, None

        @staticmethod
        def jvp(ctx, tv, *_):
            shape, (nx, ny, nz), (mx, my, mz) = ctx.layout
            (velocity,) = ctx.saved_tensors
            # d slowness = -(tv / velocity^2), velocity's layout -> (mx, my, mz) in C order -> model order x fastest
            ds = (-(tv / (velocity * velocity))).reshape(mx, my, mz).permute(2, 1, 0).contiguous().reshape(-1)
            if not ctx.return_fields:
                return ctx.tape.jvp(ds)
            dtt, df = ctx.tape.jvp(ds, return_fields=True)
            return dtt, df.reshape(df.shape[0], nz, ny, nx).permute(0, 3, 2, 1).contiguous()

    _AdjFn = RaytraceAdjointFn
    return _AdjFn


_RcvFn = None


def _receiver_function():
    global _RcvFn
    if _RcvFn is not None:
        return _RcvFn
    import torch
    from torch.autograd.function import once_differentiable

    class ReceiverTermFn(torch.autograd.Function):
        """zeros(n_data) whose derivative with respect to rcv is that of the traveltimes of the tape's rows: added to tt, it makes the
        operator differentiable in the receiver positions without touching the operator itself"""

        @staticmethod
        def forward(ctx, rcv, tape):
            ctx.tape, ctx.like = tape, (rcv.dtype, rcv.device)
            G = torch.from_numpy(tape.receiver_jacobian()).to(rcv.device)
            ctx.save_for_backward(G)
            return torch.zeros(tape.n_data, dtype=G.dtype, device=rcv.device)

        @staticmethod
        @once_differentiable   # (second-order terms in the receiver coordinates are not implemented: raise, not a part)
        def backward(ctx, g):
            (G,) = ctx.saved_tensors
            return (g.to(G.dtype)[:, None] * G).to(dtype=ctx.like[0], device=ctx.like[1]), None

        @staticmethod
        def jvp(ctx, t_rcv, _):
            tape = ctx.tape
            d = t_rcv.detach().cpu().numpy()
            drcv = np.zeros((tape.n_rcv_points, 4), dtype=tape.dtype)   # (a fresh tape: one receiver point per tape row)
            drcv[:, 1:] = d[tape._rows, :3]
            return torch.from_numpy(tape.jvp_receiver(drcv)).to(t_rcv.device)

    _RcvFn = ReceiverTermFn
    return _RcvFn


def _split_rcv(rcv):
    """(rcv as a numpy array, rcv itself if it is a torch tensor the result has to be differentiated by, else None)"""
    if not type(rcv).__module__.startswith('torch'):
        return np.asarray(rcv), None
    import torch.autograd.forward_ad as fwad

    wanted = rcv.requires_grad or fwad.unpack_dual(rcv).tangent is not None
    return rcv.detach().cpu().numpy(), (rcv if wanted else None)


def _with_receiver_term(out, rcv_t, holder, return_fields):
    """tt + the receiver term where rcv is to be differentiated by (fl(a + b) in forward mode; the values of tt are not changed)"""
    if rcv_t is None:
        return out
    if rcv_t.dim() != 2 or rcv_t.shape[1] != 3:
        raise ValueError('rcv should be (n, 3) to be differentiated by, got shape %s' % (tuple(rcv_t.shape),))
    tt = out[0] if return_fields else out
    term = _receiver_function().apply(rcv_t, holder[0]).to(tt.device)
    return (tt + term, out[1]) if return_fields else tt + term


def _check_wrt(grid, wrt):
    """the refusals of Grid3d.raytrace_adjoint, before the model is set"""
    if wrt not in ('nodes', 'cells'):
        raise ValueError("wrt should be 'nodes' or 'cells', got %r" % (wrt,))
    if grid._ndim != 3:
        raise NotImplementedError('the adjoint-state gradient is implemented for 3-D grids only')
    if grid.cell_slowness and wrt == 'nodes':
        raise NotImplementedError("the adjoint-state gradient with respect to node slowness is not implemented for grids with slowness "
                                  "defined for cells: wrt='cells' gives the gradient with respect to the cells")
    if not grid.cell_slowness and wrt == 'cells':
        raise ValueError("wrt='cells' needs a grid with slowness defined for cells (cell_slowness=1); this grid has it at the nodes")


def _model_dims(grid, wrt):
    """extents of the model array velocity is laid out in: the nodes, or the cells"""
    nx, ny, nz = grid.x.size, grid.y.size, grid.z.size
    return (nx - 1, ny - 1, nz - 1) if wrt == 'cells' else (nx, ny, nz)


def raytrace_adjoint(grid, velocity, source, rcv, aggregate_src=False, return_fields=False, wrt='nodes'):
    """Traveltimes at `rcv` (interpolated, as with tt_from_rp=0) for the model `velocity` (torch tensor, node grid layout; cell layout
    with wrt='cells' on a cell grid), differentiable with respect to velocity by the adjoint-state method: backward =
    -(FieldTape.vjp) / velocity**2, the exact derivative of the returned values.  return_fields=True: (tt, fields) with the
    (n_events, nx, ny, nz) traveltime fields, differentiable as well."""
    _check_wrt(grid, wrt)
    source = np.asarray(source)
    rcv, rcv_t = _split_rcv(rcv)
    holder = []
    out = _adjoint_function().apply(velocity, grid, source, rcv, bool(aggregate_src), bool(return_fields), wrt, holder)
    return _with_receiver_term(out, rcv_t, holder, return_fields)


def _events_function():
    global _EvFn
    if _EvFn is not None:
        return _EvFn
    import torch
    from torch.autograd.function import once_differentiable

    class RaytraceEventsFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, velocity, events, grid, event_of_row, rcv, return_fields, wrt, holder):
            grid.set_velocity(velocity.detach().cpu().numpy())
            ev = events.detach().cpu().numpy().astype(np.float64)
            # the 5-column source form of _split_sources: (event number, t0, x, y, z) per rcv row; events are taken in ascending number
            source = np.column_stack([event_of_row.astype(np.float64), ev[event_of_row]])
            tt, tape = grid.raytrace_adjoint(source, rcv, wrt=wrt)
            holder.append(tape)   # (for the receiver term: _with_receiver_term)
            nx, ny, nz = grid.x.size, grid.y.size, grid.z.size
            ctx.tape = tape
            ctx.layout = (tuple(velocity.shape), (nx, ny, nz), _model_dims(grid, wrt))
            ctx.save_for_backward(velocity, events)
            ctx.save_for_forward(velocity)
            ctx.return_fields = return_fields
            out = torch.from_numpy(tt).to(velocity.device)
            if not return_fields:
                return out
            f = np.stack([tape.field(e).reshape(nz, ny, nx).transpose(2, 1, 0) for e in range(tape.n_events)])
            return out, torch.from_numpy(np.ascontiguousarray(f)).to(velocity.device)

        @staticmethod
        @once_differentiable   # (second derivatives with respect to the source points, and mixed ones, are not implemented: raise, not a part)
        def backward(ctx, g, gf=None):
            shape, (nx, ny, nz), (mx, my, mz) = ctx.layout
            velocity, events = ctx.saved_tensors
            fc = None
            if gf is not None:   # (n_events, nx, ny, nz) in C order -> node order x fastest
                fc = gf.permute(0, 3, 2, 1).contiguous().reshape(gf.shape[0], -1)
            gn, gs = ctx.tape.vjp(g.contiguous(), fc, return_source_grad=True)
            gs_v = gn.reshape(mz, my, mx).permute(2, 1, 0).contiguous().reshape(shape).to(velocity.dtype)
            return -gs_v / (velocity * velocity), gs.to(device=events.device, dtype=events.dtype), None, None, None, None, None, None

        @staticmethod
        def jvp(ctx, tv, te, *_):
            shape, (nx, ny, nz), (mx, my, mz) = ctx.layout
            (velocity,) = ctx.saved_tensors
            parts = []
            if tv is not None:
                ds = (-(tv / (velocity * velocity))).reshape(mx, my, mz).permute(2, 1, 0).contiguous().reshape(-1)
                parts.append(ctx.tape.jvp(ds, return_fields=ctx.return_fields))
            if te is not None:
                parts.append(ctx.tape.jvp_source(te.to(velocity.device), return_fields=ctx.return_fields))
            if not ctx.return_fields:
                return parts[0] if len(parts) == 1 else parts[0] + parts[1]
            dtt, df = parts[0] if len(parts) == 1 else (parts[0][0] + parts[1][0], parts[0][1] + parts[1][1])
            return dtt, df.reshape(df.shape[0], nz, ny, nx).permute(0, 3, 2, 1).contiguous()

    _EvFn = RaytraceEventsFn
    return _EvFn


def raytrace_events(grid, velocity, events, event_of_row, rcv, return_fields=False, wrt='nodes'):
    """Traveltimes at `rcv` (interpolated, as with tt_from_rp=0) of row r for the event event_of_row[r] of `events`, an (n_events, 4)
    torch tensor of (t0, x, y, z); differentiable with respect to `velocity` (as raytrace_adjoint) and `events` (d tt / d origin time
    and position, exact, FieldTape.vjp(..., return_source_grad=True)).  return_fields=True: (tt, fields) with the (n_events, nx, ny, nz)
    traveltime fields, differentiable as well.  wrt='cells': a cell grid, velocity in the cell layout."""
    _check_wrt(grid, wrt)
    rcv, rcv_t = _split_rcv(rcv)
    event_of_row = np.asarray(event_of_row)
    if events.dim() != 2 or events.shape[1] != 4:
        raise ValueError('events should be (n_events, 4): t0, x, y, z; got shape %s' % (tuple(events.shape),))
    if event_of_row.ndim != 1 or rcv.ndim != 2 or event_of_row.shape[0] != rcv.shape[0] or event_of_row.dtype.kind not in 'iu':
        raise ValueError('event_of_row should hold one integer per rcv row')
    if not np.array_equal(np.unique(event_of_row), np.arange(events.shape[0])):
        raise ValueError('event_of_row should name events 0 .. %d, every one of them at least once' % (events.shape[0] - 1))
    holder = []
    out = _events_function().apply(velocity, events, grid, event_of_row.astype(np.int64), rcv, bool(return_fields), wrt, holder)
    return _with_receiver_term(out, rcv_t, holder, return_fields)


def _apply_map(grid, t, model_shape, prolong):
    """P (prolong) or P^T of the tensor t in C order of its grid -- (mx, my, mz) model nodes or (nx, ny, nz) nodes -- through the
    grid's own kernels; the result in C order of the other grid, in t's dtype, where t lives"""
    m3 = grid._model_shape(model_shape)
    n3 = (grid.x.size, grid.y.size, grid.z.size)
    src, dst = (m3, n3) if prolong else (n3, m3)
    if t.numel() != src[0] * src[1] * src[2]:
        raise ValueError('%s should hold %d x %d x %d values, got shape %s' % (('m' if prolong else 'g',) + tuple(src) + (tuple(t.shape),)))
    flat = t.detach().reshape(src).permute(2, 1, 0).contiguous().reshape(-1)   # C order -> x fastest
    out = (grid.prolong if prolong else grid.restrict)(flat, m3)
    return out.reshape(dst[2], dst[1], dst[0]).permute(2, 1, 0).contiguous().to(device=t.device, dtype=t.dtype)


def _map_functions():
    global _MapFns
    if _MapFns is not None:
        return _MapFns
    import torch

    class ProlongFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, m, grid, model_shape):
            ctx.grid, ctx.model_shape, ctx.in_shape = grid, model_shape, tuple(m.shape)
            return _apply_map(grid, m, model_shape, True)

        @staticmethod
        def backward(ctx, g):   # (through the public operator: differentiable again)
            return restrict(ctx.grid, g, ctx.model_shape).reshape(ctx.in_shape), None, None

        @staticmethod
        def jvp(ctx, tm, *_):
            return _apply_map(ctx.grid, tm, ctx.model_shape, True)

    class RestrictFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, g, grid, model_shape):
            ctx.grid, ctx.model_shape, ctx.in_shape = grid, model_shape, tuple(g.shape)
            return _apply_map(grid, g, model_shape, False)

        @staticmethod
        def backward(ctx, gm):
            return prolong(ctx.grid, gm, ctx.model_shape).reshape(ctx.in_shape), None, None

        @staticmethod
        def jvp(ctx, tg, *_):
            return _apply_map(ctx.grid, tg, ctx.model_shape, False)

    _MapFns = (ProlongFn, RestrictFn)
    return _MapFns


def prolong(grid, m, model_shape):
    """P m: the torch tensor m of values at the (mx, my, mz) nodes of a coarse model grid (that shape, or flat in C order), interpolated
    trilinearly onto the nodes of the 3-D node grid `grid`: an (nx, ny, nz) tensor in m's dtype where m lives (Grid3d.prolong computes
    it in the grid dtype).  Differentiable: the backward is restrict, forward mode is prolong of the tangent."""
    return _map_functions()[0].apply(m, grid, tuple(model_shape))


def restrict(grid, g, model_shape):
    """P^T g: the transpose of prolong applied to an (nx, ny, nz) tensor (or flat in C order): (mx, my, mz).  The backward is prolong."""
    return _map_functions()[1].apply(g, grid, tuple(model_shape))
