"""ttcr_amd.autograd -- traveltimes as a differentiable torch operator (no ttcrpy counterpart).

    tt = ttcr_amd.autograd.raytrace(grid, velocity, source, rcv, aggregate_src=False)

`grid` is a 3-D node grid (Grid3d(..., cell_slowness=0)); `velocity` a torch tensor of node velocities, shape (nx, ny, nz) or flat in
C order (what Grid3d.set_velocity reads).  The forward sets the model as set_velocity does (through the host: 1 / velocity in numpy,
then the grid dtype) and runs grid.raytrace_tape; tt is a tensor of the grid dtype on velocity's device, bit-equal to
raytrace(..., compute_M=True)[0].  The backward is M^T g (MTape.vjp, on the device) permuted to velocity's layout, where M is the
reference's matrix of d tt / d velocity with the rays held fixed: the gradient of the ray-frozen (linearised) problem, not the exact
derivative of the returned tt.  A model in slowness composes in torch: raytrace(grid, 1 / s, ...).

    tt = ttcr_amd.autograd.raytrace_adjoint(grid, velocity, source, rcv, aggregate_src=False, return_fields=False)

is the same operator with the EXACT derivative: the forward runs grid.raytrace_adjoint (interpolated receiver traveltimes, as a grid
with tt_from_rp=0 returns them; 3-D node grids with weno=0), the backward is the adjoint-state gradient FieldTape.vjp -- the derivative
of the returned tt through the solver's own first-order update -- times d slowness / d velocity = -1 / velocity**2, in velocity's layout.
With return_fields=True it returns (tt, fields), fields the (n_events, nx, ny, nz) traveltime fields, differentiable too: a loss on the
grid traveltimes has a gradient.  Forward mode works as well (torch.autograd.forward_ad): the tangent of the outputs for a velocity
tangent tv is FieldTape.jvp(-(tv / velocity**2)), J v of the same linearisation, in the layout of the outputs.

torch is imported when this module is used, never by `import ttcr_amd`.
"""
import numpy as np

_Fn = None
_AdjFn = None


def _function():
    global _Fn
    if _Fn is not None:
        return _Fn
    import torch

    class RaytraceFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, velocity, grid, source, rcv, aggregate_src):
            grid.set_velocity(velocity.detach().cpu().numpy())
            tt, tape = grid.raytrace_tape(source, rcv, aggregate_src=aggregate_src)
            ctx.tape = tape
            ctx.layout = (tuple(velocity.shape), velocity.dtype, (grid.x.size, grid.y.size, grid.z.size))
            return torch.from_numpy(tt).to(velocity.device)

        @staticmethod
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

    class RaytraceAdjointFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, velocity, grid, source, rcv, aggregate_src, return_fields):
            grid.set_velocity(velocity.detach().cpu().numpy())
            tt, tape = grid.raytrace_adjoint(source, rcv, aggregate_src=aggregate_src)
            nx, ny, nz = grid.x.size, grid.y.size, grid.z.size
            ctx.tape = tape
            ctx.layout = (tuple(velocity.shape), (nx, ny, nz))
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
            shape, (nx, ny, nz) = ctx.layout
            (velocity,) = ctx.saved_tensors
            fc = None
            if gf is not None:   # (n_events, nx, ny, nz) in C order -> node order x fastest
                fc = gf.permute(0, 3, 2, 1).contiguous().reshape(gf.shape[0], -1)
            gn = ctx.tape.vjp(g.contiguous(), fc)
            # node order x fastest -> (nx, ny, nz) in C order -> velocity's layout; d slowness / d velocity = -1 / velocity^2
            gs = gn.reshape(nz, ny, nx).permute(2, 1, 0).contiguous().reshape(shape).to(velocity.dtype)
            return -gs / (velocity * velocity), None, None, None, None, None

        @staticmethod
        def jvp(ctx, tv, *_):
            shape, (nx, ny, nz) = ctx.layout
            (velocity,) = ctx.saved_tensors
            # d slowness = -(tv / velocity^2), velocity's layout -> (nx, ny, nz) in C order -> node order x fastest
            ds = (-(tv / (velocity * velocity))).reshape(nx, ny, nz).permute(2, 1, 0).contiguous().reshape(-1)
            if not ctx.return_fields:
                return ctx.tape.jvp(ds)
            dtt, df = ctx.tape.jvp(ds, return_fields=True)
            return dtt, df.reshape(df.shape[0], nz, ny, nx).permute(0, 3, 2, 1).contiguous()

    _AdjFn = RaytraceAdjointFn
    return _AdjFn


def raytrace_adjoint(grid, velocity, source, rcv, aggregate_src=False, return_fields=False):
    """Traveltimes at `rcv` (interpolated, as with tt_from_rp=0) for the model `velocity` (torch tensor, node grid layout), differentiable
    with respect to velocity by the adjoint-state method: backward = -(FieldTape.vjp) / velocity**2, the exact derivative of the returned
    values.  return_fields=True: (tt, fields) with the (n_events, nx, ny, nz) traveltime fields, differentiable as well."""
    if grid._ndim != 3:
        raise NotImplementedError('the adjoint-state gradient is implemented for 3-D grids only')
    if grid.cell_slowness:
        raise NotImplementedError('the adjoint-state gradient is not implemented for grids with slowness defined for cells')
    source = np.asarray(source)
    rcv = np.asarray(rcv)
    return _adjoint_function().apply(velocity, grid, source, rcv, bool(aggregate_src), bool(return_fields))
