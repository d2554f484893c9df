"""ttcr_amd.autograd -- traveltimes as a differentiable torch operator (no ttcrpy counterpart).

    tt = ttcr_amd.autograd.raytrace(grid, velocity, source, rcv, aggregate_src=False)

`grid` is a 3-D node grid (Grid3d(..., cell_slowness=0)); `velocity` a torch tensor of node velocities, shape (nx, ny, nz) or flat in
C order (what Grid3d.set_velocity reads).  The forward sets the model as set_velocity does (through the host: 1 / velocity in numpy,
then the grid dtype) and runs grid.raytrace_tape; tt is a tensor of the grid dtype on velocity's device, bit-equal to
raytrace(..., compute_M=True)[0].  The backward is M^T g (MTape.vjp, on the device) permuted to velocity's layout, where M is the
reference's matrix of d tt / d velocity with the rays held fixed: the gradient of the ray-frozen (linearised) problem, not the exact
derivative of the returned tt.  A model in slowness composes in torch: raytrace(grid, 1 / s, ...).

torch is imported when this module is used, never by `import ttcr_amd`.
"""
import numpy as np

_Fn = None


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
