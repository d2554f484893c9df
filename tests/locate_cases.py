"""Cases of the grid-search location tests (tests/test_locate.py on oracle fields, tests/test_locate_gpu.py on the device's own fields):
the 9 x 8 x 10 node grid with five surface stations off the nodes, the mirror-tie grid, and the picks made from fields."""
import numpy as np

NN = (9, 8, 10)
DX = 0.5
ZERO = (0.0, 0.0, 0.0)
# five surface stations (z = 0) off the nodes, in node-index units
STATIONS = [[0.3, 0.4, 0.0], [7.6, 0.7, 0.0], [4.4, 3.6, 0.0], [0.6, 6.5, 0.0], [7.3, 6.2, 0.0]]
TRUE_NODES = (463, 0, 719, 656)   # interior, both far corners, an edge
T_ORIGIN = 12.5

# the mirror tie: homogeneous slowness, stations on nodes of the node plane k = 5, a hypocentre on the plane k = 7.  The oracle's fields
# of such stations are mirror-symmetric about the plane to the bit (checked for planes of all three axes; z is used), so the node on
# k = 3 has the same phi as the true one and the lower index
MIRROR_PLANE = 5
MIRROR_STATIONS = [[6, 6, 5], [7, 3, 5], [5, 2, 5], [0, 2, 5]]
MIRROR_TRUE = (4, 3, 7)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def node_of(nn, i, j, k):
    return (k * nn[1] + j) * nn[0] + i


def model(nn, kind="gradient"):
    """node slowness, flat, x fastest: `gradient` = velocity 2 + 0.4 z (z in km, DX per node) with 10 % roughness; `smooth` the same
    without the roughness; `homogeneous` 0.5"""
    n = int(np.prod(nn))
    if kind == "homogeneous":
        return np.full(n, 0.5)
    k = np.arange(n) // (nn[0] * nn[1])
    s = 1.0 / (2.0 + 0.4 * DX * k)
    if kind == "gradient":
        s = s * (1.0 + 0.1 * np.random.default_rng(17).uniform(-1.0, 1.0, n))
    return s


def station_points(stations, dx=DX, origin=ZERO):
    return np.asarray(origin, dtype=np.float64) + np.asarray(stations, dtype=np.float64) * dx


def oracle_fields(dt, nn, s, stations, dx=DX, origin=ZERO):
    """the oracle's field of every station, converged (eps = 1e-15): (n_stations, n_nodes) in dt"""
    from oracle import oracle as O

    nc = tuple(n - 1 for n in nn)
    return np.stack([O.solve3d(dt, nc, dx, origin, np.asarray(s, dtype=dt), p[None, :], eps=1e-15, maxit=200)["tt"]
                     for p in station_points(stations, dx, origin)])


def picks_at(T, values_at, fields=None, t_origin=0.0, weights=None, hypo=0):
    """picks of one hypocentre: time = t_origin + the value of every field in `fields` (default: all) at `values_at` -- a node index, or an
    array of one value per field of T --, weight 1 + 0.5 f unless given.  Returns (pick_hypo, pick_field, pick_time, pick_weight)."""
    T = np.asarray(T)
    fields = np.arange(T.shape[0]) if fields is None else np.asarray(fields, dtype=np.int64)
    v = T[fields, values_at].astype(np.float64) if np.ndim(values_at) == 0 else np.asarray(values_at, dtype=np.float64)[fields]
    w = 1.0 + 0.5 * fields if weights is None else np.asarray(weights, dtype=np.float64)
    return np.full(fields.size, hypo, dtype=np.int64), fields, t_origin + v, w


def join(*picks):
    """several hypocentres' picks in one call, interleaved (pick i of every hypocentre in turn) so that the grouping has work to do"""
    order = np.argsort(np.concatenate([np.arange(p[0].size) for p in picks]), kind="stable")
    return tuple(np.concatenate([p[c] for p in picks])[order] for c in range(4))


def base_picks(T):
    """the base case: hypocentres 0 .. 3 at TRUE_NODES with all fields, 4 .. 7 the same with T_ORIGIN added and four of the five stations
    (a different one left out each time), 8 one pick of weight 1 (phi == 0 everywhere: the lowest node wins)"""
    ps = [picks_at(T, m, hypo=q) for q, m in enumerate(TRUE_NODES)]
    nf = np.asarray(T).shape[0]
    ps += [picks_at(T, m, fields=[f for f in range(nf) if f != q % nf], t_origin=T_ORIGIN, hypo=4 + q) for q, m in enumerate(TRUE_NODES)]
    ps.append(picks_at(T, TRUE_NODES[0], fields=[2], weights=[1.0], hypo=8))
    return join(*ps)
