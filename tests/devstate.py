"""Device-side copies and comparisons of a Tau3D handle's state: the six fields are copied device to device (tau3d_state_ptrs +
hipMemcpy) into torch int32 tensors on the GPU and compared there, so that a 512^3 state (3.2 GB) is never downloaded."""
import ctypes as C

import torch

FIELDS = ("xi", "phix", "phiy", "phiz", "lam", "zet")


def hip():
    """the HIP runtime the engine is bound to (fluid_sims_amd.taueng), with hipMemcpy's signature"""
    from fluid_sims_amd import taueng
    return taueng._hip_runtime()


def new_buffer(e):
    """an int32 tensor (6, nzl, ny, nx) on the GPU for snapshot()"""
    return torch.empty((6,) + tuple(e.shape), dtype=torch.int32, device="cuda")


def snapshot(e, H, dst):
    """the handle's current state into dst (int32, (6, nzl, ny, nx)), device to device: the bits of every field"""
    assert tuple(dst.shape) == (6,) + tuple(e.shape) and dst.dtype == torch.int32 and dst.is_contiguous()
    ptrs, _ = e.state_ptrs()
    e.sync()
    nb = dst[0].numel() * 4
    for m in range(6):
        assert H.hipMemcpy(dst[m].data_ptr(), ptrs[m], nb, 3) == 0   # hipMemcpyDeviceToDevice
    torch.cuda.synchronize()


def first_difference(a, b):
    """None if a and b (snapshots) hold the same bits, else (field name, (z, y, x) of the first differing cell, differing cells)"""
    for m in range(6):
        if torch.equal(a[m], b[m]):
            continue
        ne = (a[m] != b[m]).reshape(-1)
        i = int(torch.argmax(ne.to(torch.uint8)).item())
        nz, ny, nx = a[m].shape
        return FIELDS[m], (i // (ny * nx), i // nx % ny, i % nx), int(ne.sum().item())
    return None


def assert_same_state(a, b, what):
    d = first_difference(a, b)
    assert d is None, f"{what}: field {d[0]} differs first at (z, y, x) = {d[1]}, in {d[2]} cells"


def clock_tuple(e):
    c = e.clock()
    return tuple(getattr(c, n) for n, _ in c._fields_)
