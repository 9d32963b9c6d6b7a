"""The 3D step's exact shortcuts at the benchmarked size, 512^3: the uniform-region exits (k_flux_xy / k_update_z), the predicted-uniform
tile list (k_tile_predict) and the per-field store skip of predicted tiles (k_fill_z) against the same step with every face evaluated
(TAU3D_UNIFORM_EXITS=0), byte for byte over the six fields and the clock — on bench.py's headline start, on the impulsive start from
rest and on the late state behind value_late (2 500 steps of the ramped start).  The states are compared on the device
(tests/devstate.py), and at every comparison point the counters show that each shortcut ran on the handle being checked, so that the
identity cannot reduce to two runs of the full path.

Two handles step in lockstep (about 6.5 GB each); the headline case adds a third in verifying mode (TAU3D_TILE_LIST=2).
Measured on the MI355X: about 21 s for the file, 20 s of it the late state (2 x 2 500 steps)."""
import pytest

from tests.devstate import assert_same_state, clock_tuple, hip, new_buffer, snapshot

pytestmark = pytest.mark.gpu
N = 512


def _handle(eng, monkeypatch, env, mode, bench_clock):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        e = eng.Tau3D(N)         # (the variables are read by tau3d_create)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    assert e.is_split()
    e.init(mode)
    if bench_clock:
        e.set_clock(0.02, 1e-4)
    return e


def _shortcuts_ran(e, what):
    """the counters of the last step of the listed handle: exits taken, a list shorter than the grid, field stores skipped"""
    flagged, tiles, on = e.uniform_tiles()
    mode, listed, ltiles, _, _ = e.tile_list_stats()
    skipped, pred = e.store_skip_stats()
    ncell = N ** 3
    print(f"{what}: uniform tiles {flagged / tiles:.3f}, listed tiles {listed / ltiles:.3f}, predicted cells {pred / ncell:.3f}, "
          f"stores skipped {sum(skipped) / (6 * ncell):.3f} of all field stores", flush=True)
    assert on and flagged > 0, f"{what}: no uniform-region exit was taken"
    assert mode == 1 and 0 <= listed < ltiles, f"{what}: no tile list shorter than the grid (mode {mode}, listed {listed} of {ltiles})"
    assert pred > 0 and sum(skipped) > 0, f"{what}: no field store was skipped ({skipped} of {pred} predicted cells)"


def _lockstep(eng, monkeypatch, mode, bench_clock, points, verify=False):
    H = hip()
    a = _handle(eng, monkeypatch, {}, mode, bench_clock)
    b = _handle(eng, monkeypatch, {"TAU3D_UNIFORM_EXITS": "0"}, mode, bench_clock)
    v = _handle(eng, monkeypatch, {"TAU3D_TILE_LIST": "2"}, mode, bench_clock) if verify else None
    sa, sb = new_buffer(a), new_buffer(a)
    done = 0
    try:
        for p in points:
            for h in (a, b, v):
                if h is not None:
                    h.step(p - done)
            done = p
            what = f"init({mode}){' + bench clock' if bench_clock else ''}, step {p}"
            _shortcuts_ran(a, what)
            assert b.uniform_tiles()[2] is False and b.tile_list_stats()[0] == 0
            ca, cb = clock_tuple(a), clock_tuple(b)
            assert ca == cb, f"{what}: clock {ca} (shortcuts) != {cb} (every face)"
            snapshot(a, H, sa)
            snapshot(b, H, sb)
            assert_same_state(sa, sb, f"{what}: shortcuts against every face")
            if v is not None:
                m, _, _, checked, mismatches = v.tile_list_stats()
                assert m == 2 and checked > 0 and mismatches == 0, f"{what}: verifying mode checked {checked}, {mismatches} mismatches"
                assert clock_tuple(v) == ca
                snapshot(v, H, sb)
                assert_same_state(sa, sb, f"{what}: list against verifying mode")
    finally:
        for h in (a, b, v):
            if h is not None:
                h.close()
        del sa, sb
        import torch
        torch.cuda.empty_cache()


def test_headline_start_512(eng, monkeypatch):
    """bench.py's setup (init(1), clock (0.02, 1e-4)): after the driver's 5 warm-up + 20 timed steps and bench.py's default 10 + 20;
    a third handle verifies every prediction (TAU3D_TILE_LIST=2)"""
    _lockstep(eng, monkeypatch, 1, True, (25, 30), verify=True)


def test_impulsive_start_512(eng, monkeypatch):
    """init(0): the body and the inflow start from a gas at rest, 45 steps"""
    _lockstep(eng, monkeypatch, 0, False, (45,))


def test_late_state_512(eng, monkeypatch):
    """the state behind bench.py's value_late: the ramped start (init(0), default clock) for 2 500 steps, checked at 300, 1 000, 2 500"""
    _lockstep(eng, monkeypatch, 0, False, (300, 1000, 2500))
