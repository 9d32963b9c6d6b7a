"""Predicted-tile stores skipped field by field (k_tile_predict's bits 2-7 of the dzero word, k_fill_z): the same bits as a step
that stores every field, and the tile list's flags dropped when the fused kernel steps in between."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("shape,mode,steps", [((160, 128, 96), 1, 30), ((256, 192, 128), 1, 40), ((256, 256, 64), 0, 120)])
def test_partial_store_masks_change_no_bit(eng, monkeypatch, shape, mode, steps):
    """List on (predicted tiles skip the fields the buffer holds) against TAU3D_TILE_LIST=0 (no prediction: every store) and
    TAU3D_UNIFORM_EXITS=0, byte for byte over the fields and the clock, with a dent uploaded mid-run.  From tau3d_store_skip_stats:
    on the impulsive start some field was skipped on cells where not all six were — the masks were partial, so the identity
    covers them."""
    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = eng.Tau3D(*shape)
        e.set_split(True)
        e.init(mode)
        if mode:
            e.set_clock(0.02, 1e-4)
        out, partial, skipped = [], 0, 0
        for i, k in enumerate((2, steps - 2, 3, 5)):
            for _ in range(k):
                e.step(1)
                cnt, pred = e.store_skip_stats()
                assert all(0 <= c <= pred for c in cnt)
                partial += max(cnt) - min(cnt)
                skipped += sum(cnt)
            c = e.clock()
            st = e.download()
            out.append((st, (c.t, c.d_tau, c.maxs)))
            if i == 1:      # a dent in the far corner of the grid, away from the body and the sponges: uniform there on these starts
                st = [f.copy() for f in st]
                st[4][shape[2] - 5, shape[1] - 9, shape[0] // 2 + 7] += 0.25
                e.upload(st)
        e.close()
        for k in env:
            monkeypatch.delenv(k)
        return out, partial, skipped
    (a, partial, skipped), (b, _, sb), (x, _, sx) = (run({}), run({"TAU3D_TILE_LIST": "0"}),
                                                     run({"TAU3D_UNIFORM_EXITS": "0"}))
    for (sa, ca), (sb_, cb), (sx_, cx) in zip(a, b, x):
        assert ca == cb == cx
        _same(sa, sb_)
        _same(sa, sx_)
    assert sb == 0 and sx == 0   # (no list: nothing predicted, nothing skipped)
    print(shape, "mode", mode, "field stores skipped", skipped, "of which beside a field that was stored", partial)
    assert skipped > 0
    if mode == 1:
        assert partial > 0, "no partial mask occurred: the identity says nothing about them"


def test_split_fused_split_drops_the_list(eng, monkeypatch):
    """split steps -> two fused steps -> split steps: the flags the first split steps left must not be trusted after the fused
    ones (the buffer parity is the same again after two of them).  Byte for byte against TAU3D_TILE_LIST=0."""
    shape = (160, 128, 96)
    def run(tl):
        monkeypatch.setenv("TAU3D_TILE_LIST", tl)
        e = eng.Tau3D(*shape)
        e.set_split(True)
        e.init(1)
        e.set_clock(0.02, 1e-4)
        out = []
        for split, k in ((True, 12), (False, 2), (True, 6)):
            e.set_split(split)
            e.step(k)
            c = e.clock()
            out.append((e.download(), (c.t, c.d_tau, c.maxs)))
        e.close()
        return out
    a, b = run("1"), run("0")
    for (sa, ca), (sb, cb) in zip(a, b):
        assert ca == cb
        _same(sa, sb)
