"""Writes through tau3d_state_ptrs followed by tau3d_state_written (include/taueng.h: the contract for a caller that writes the state
or the solid mask through the pointers): the tile list is dropped, the field range that picks the WENO weight form is measured
again, and k_flux_xy's static solid-free tile flags are rebuilt from the mask — each checked byte for byte against a step that
keeps no such state, or against the CPU oracle."""
import numpy as np
import pytest

from tests.parity import assert_parity

pytestmark = pytest.mark.gpu
FIELDS = ("xi", "phix", "phiy", "phiz", "lam", "zet")


def _create(eng, monkeypatch, shape, env=None, params=None):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return eng.Tau3D(*shape, params=params)     # (the variables are read by tau3d_create)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _write_cell(e, field, zyx, value):
    """one cell of the current state through the device pointer of tau3d_state_ptrs"""
    ptrs, _ = e.state_ptrs()
    off = int(np.ravel_multi_index(zyx, e.shape)) * 4
    e.write_device(ptrs[field], np.array([value], np.float32), off)


def _same(a, b, what):
    for m, (x, y) in enumerate(zip(a, b)):
        ne = x.view(np.uint32) != y.view(np.uint32)
        if ne.any():
            raise AssertionError(f"{what}: field {FIELDS[m]} differs first at (z, y, x) = {tuple(int(i) for i in np.argwhere(ne)[0])}, "
                                 f"in {int(ne.sum())} cells")


def _uniform_cell(prev, cur, shape):
    """a cell in the middle of a tile whose 3 x 3 tile neighbourhood, with its 3-cell x / y halo, over planes z - 4 .. z + 4 holds one
    encoded state in all six fields, both in the state before the last step and after it: k_tile_predict flags the tile for the
    next step (its neighbourhood is one state) and every field's store is skipped there (the output buffer, the state before,
    already holds it)"""
    nx, ny, nz = shape
    for z in (nz - 6, nz // 2, 5):
        for ty in range(ny // 16 - 2, 0, -1):
            for tx in range(nx // 32 - 2, 0, -1):
                sl = (slice(z - 4, z + 5), slice(16 * (ty - 1) - 3, 16 * (ty + 2) + 3), slice(32 * (tx - 1) - 3, 32 * (tx + 2) + 3))
                if all((st[m][sl].view(np.uint32) == st[m][sl].view(np.uint32).flat[0]).all() for st in (prev, cur) for m in range(6)):
                    return (z, 16 * ty + 8, 32 * tx + 16)
    raise AssertionError(f"{shape}: no uniform tile neighbourhood to dent")


@pytest.mark.parametrize("shape", [(160, 128, 96), (256, 192, 128)])
@pytest.mark.parametrize("twice", [False, True], ids=["one_write", "two_steps_in_a_row"])
def test_dent_inside_a_predicted_region(eng, monkeypatch, shape, twice):
    """Ramped start, 30 steps; then a dent in xi (and, in the second case, a dent in phix the step after) of a cell deep inside a
    region that k_tile_predict flags and whose stores k_fill_z skips — written through the pointer + state_written.  1, 2 and 10
    more steps: fields and clock byte for byte against the same writes with no tile list (TAU3D_TILE_LIST=0), with every face
    evaluated (TAU3D_UNIFORM_EXITS=0), and against the same dents made with tau3d_upload_state."""
    warm = 30
    # where to dent: found on a run with the list (the states before and after the last warm-up step)
    e = _create(eng, monkeypatch, shape)
    e.set_split(True)
    e.init(0)
    e.step(warm - 1)
    prev = e.download()
    e.step(1)
    cur = e.download()
    _, listed, tiles, _, _ = e.tile_list_stats()
    skipped, pred = e.store_skip_stats()
    e.close()
    cell = _uniform_cell(prev, cur, shape)
    print(shape, "dent at", cell, f"listed tiles {listed / tiles:.3f}, stores skipped per field {[round(s / max(pred, 1), 3) for s in skipped]}")
    assert 0 <= listed < tiles and skipped[0] > 0 and skipped[1] > 0

    def run(env, via_ptr):
        e = _create(eng, monkeypatch, shape, env)
        e.set_split(True)
        e.init(0)
        e.step(warm)
        for i, (field, d) in enumerate(((0, 0.25), (1, -0.125))[:2 if twice else 1]):
            if i:
                e.step(1)
            st = e.download()
            v = np.float32(st[field][cell] + np.float32(d))
            if via_ptr:
                _write_cell(e, field, cell, v)
                e.state_written()
            else:
                st[field][cell] = v
                e.upload(st)
        out = []
        for k in (1, 1, 8):
            e.step(k)
            c = e.clock()
            out.append((e.download(), tuple(getattr(c, n) for n, _ in c._fields_)))
        skipped, _ = e.store_skip_stats()
        e.close()
        return out, sum(skipped)

    (a, sa), (b, _), (x, _), (u, _) = (run({}, True), run({"TAU3D_TILE_LIST": "0"}, True),
                                       run({"TAU3D_UNIFORM_EXITS": "0"}, True), run({}, False))
    assert sa > 0, "after the writes the list came back: stores were skipped again"
    for i, ((s0, c0), (s1, c1), (s2, c2), (s3, c3)) in enumerate(zip(a, b, x, u)):
        what = f"{shape} dent {'twice' if twice else 'once'}, {(1, 2, 10)[i]} steps after"
        assert c0 == c1 == c2 == c3, (what, c0, c1, c2, c3)
        _same(s0, s1, what + ": list against no list")
        _same(s0, s2, what + ": list against every face")
        _same(s0, s3, what + ": pointer write against upload")


@pytest.mark.parametrize("shape,split", [((48, 40, 24), False), ((160, 128, 24), True)])
def test_field_range_through_the_pointer(eng, oracle_built, monkeypatch, shape, split):
    """a velocity beyond the fast WENO window (|u| > 2.5e3) written into one free-stream cell: after state_written the handle's written
    range holds it, the next step takes the reciprocal weights, and that step matches the CPU oracle (split and fused)"""
    from tests.test_gpu_tau3d import oracle_one_step
    nx, ny, nz = shape
    e = _create(eng, monkeypatch, shape)
    e.set_split(split)
    e.init(1)
    e.set_clock(0.02, 1e-4)
    e.step(12)
    dt = float(e.clock().dt)
    assert e.field_range()[2], "the developed state must be inside the fast window"
    cell = (nz // 2, ny - 4, nx - 40)
    assert e.solid()[cell] == 0
    u_ref = e.params.u_ref
    big = np.float32(np.arcsinh(3.0e3 / u_ref))                 # phix = asinh(u / u_ref): u = 3e3
    _write_cell(e, 1, cell, big)
    e.state_written()
    rng = e.field_range()
    assert rng[1] >= 2.9e3, f"the written range does not hold the new cell: {rng}"
    st = e.download()
    assert st[1][cell] == big
    o = oracle_built.Oracle3D(nx, ny, nz)
    h = 1e-3 * dt
    want, m_want = oracle_one_step(oracle_built, o, st, h, 1.0)
    m_got = e.step_explicit(h, 1.0)
    got = e.download()
    rng = e.field_range()
    e.close()
    assert not rng[2] and rng[0] >= 2.9e3, f"the step did not take the reciprocal form: {rng}"
    fluid = o.interior([o.solid])[0] == 0
    r = assert_parity(got, want, mask=fluid, what=f"{shape} split={split}, reciprocal form picked by a write through the pointer")
    print(shape, "split", split, r)
    assert m_got == pytest.approx(m_want, rel=1e-5)


def test_solid_mask_through_the_pointer(eng, monkeypatch):
    """a 4 x 4 x 4 block of free-stream cells made solid through the mask pointer, its six fields set to those of a solid cell of the
    body after init, state_written, 10 steps: byte for byte against the same run with no static tile flags and no exits
    (TAU3D_XY_NOFLAGS=1 TAU3D_UNIFORM_EXITS=0: k_flux_xy reads the mask of every cell)"""
    shape = (160, 128, 96)
    nx, ny, nz = shape
    z0, y0, x0 = nz - 12, ny - 20, 3 * nx // 4

    def run(env):
        e = _create(eng, monkeypatch, shape, env)
        e.set_split(True)
        e.init(1)
        e.set_clock(0.02, 1e-4)
        sol = e.solid()
        st = e.download()
        body = np.argwhere(sol != 0)[0]
        sv = [a[tuple(body)] for a in st]
        blk = (slice(z0, z0 + 4), slice(y0, y0 + 4), slice(x0, x0 + 4))
        assert not sol[blk].any() and not sol[z0 - 4:z0 + 8, y0 - 4:y0 + 8, x0 - 4:x0 + 8].any()
        e.step(5)
        ptrs, sp = e.state_ptrs()
        mask = np.zeros((4, ny, nx), np.uint8)
        mask[:] = e.solid()[z0:z0 + 4]
        mask[:, y0:y0 + 4, x0:x0 + 4] = 1
        plane = ny * nx
        e.write_device(sp, mask, z0 * plane)
        cur = e.download()
        for m in range(6):
            f = cur[m][z0:z0 + 4].copy()
            f[:, y0:y0 + 4, x0:x0 + 4] = sv[m]
            e.write_device(ptrs[m], f, z0 * plane * 4)
        e.state_written()
        assert (e.solid()[blk] == 1).all()
        e.step(10)
        c = e.clock()
        out = (e.download(), tuple(getattr(c, n) for n, _ in c._fields_), e.uniform_tiles())
        e.close()
        return out

    a, b = run({}), run({"TAU3D_XY_NOFLAGS": "1", "TAU3D_UNIFORM_EXITS": "0"})
    assert a[1] == b[1]
    _same(a[0], b[0], "solid block through the pointer: tile flags against none")
    assert a[2][2] and a[2][0] > 0 and not b[2][2]
