"""sampler.plan_calls: the library calls a run of the sampling loop is cut into, as pure data (no GPU, no library).  Whatever
the cut points, the calls tile the run in order, hand the noise rows out consecutively, carry the single-call frame-row table in
pieces, and only the last one writes the images."""
import itertools

import numpy as np
import pytest

from synt_isic_amd.sampler import MAX_CALL_STEPS, _frame_rows, plan_calls, segment_bounds

STEPS = (1, 4, 9, 13, 130)
MASKS = {"ddpm": lambda T: [True] * (T - 1) + [False],       # every step but the last adds noise
         "ddim_eta0": lambda T: [False] * T,                   # none does
         "trailing": lambda T: [True] * T}                     # all do


def _kept_sets(T):
    subset = sorted({i for i in (2, 7, 12) if i < T} or {0})
    return {"none": [], "all": list(range(T)), "subset": subset, "last": [T - 1]}


def _cut_sets(T):
    cuts = {"single": [0, T]}
    for seg in (1, 3, 4, 64):
        for per in (3 * 32 * 32, 3 * 128 * 128):              # below and above the ramp's threshold at seg = 64
            cuts[f"segments_{seg}_{per}"] = segment_bounds(T, seg, per)
    for m in sorted({1, 4, T}):
        cuts[f"max_call_steps_{m}"] = list(range(0, T, m)) + [T]
    return cuts


@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_plan_tiles_the_run(T, mask):
    noisy = MASKS[mask](T)
    for (kname, kept), (cname, cuts), step0 in itertools.product(_kept_sets(T).items(), _cut_sets(T).items(), (0, 37)):
        plan = plan_calls(noisy, cuts, kept, step0)
        what = (T, mask, kname, cname)
        assert len(plan) == len(cuts) - 1, what
        # the calls tile [0, T) in order, none empty, none longer than the library takes
        assert [(c.a, c.b) for c in plan] == list(zip(cuts[:-1], cuts[1:])), what
        assert plan[0].a == 0 and plan[-1].b == T and all(0 < c.b - c.a <= MAX_CALL_STEPS for c in plan), what
        # z rows are handed out consecutively, one per noisy step
        assert [c.z_rows for c in plan] == [sum(noisy[c.a:c.b]) for c in plan], what
        assert [c.z_first for c in plan] == [sum(noisy[:c.a]) for c in plan], what
        assert sum(c.z_rows for c in plan) == sum(noisy), what
        # the frame-row slices are the single-call table in pieces (a table that is None there means row i for step i)
        table = _frame_rows(T, True, kept)[1]
        if not kept:
            assert all(c.rows is None for c in plan), what
        else:
            assert all(c.rows is not None and c.rows.dtype == np.int32 and c.rows.flags["C_CONTIGUOUS"] and len(c.rows) == c.b - c.a
                       for c in plan), what
            whole = np.concatenate([c.rows for c in plan])
            assert np.array_equal(whole, table if table is not None else np.arange(T)), what
            assert sorted(int(r) for r in whole if r >= 0) == list(range(len(kept))), what
        # exactly the last call carries the image output
        assert [c.last for c in plan] == [False] * (len(plan) - 1) + [True], what
        # device noise: step i of call k has step index step0 + a_k + i
        assert [c.step0 for c in plan] == [step0 + c.a for c in plan], what


def test_single_call_plan():
    (c,) = plan_calls([True, True, False], [0, 3], [0, 2])
    assert (c.a, c.b, c.z_first, c.z_rows, c.step0, c.last) == (0, 3, 0, 2, 0, True) and c.rows.tolist() == [0, -1, 1]


def test_plan_refuses_cuts_that_do_not_tile():
    for cuts in ([0], [1, 4], [0, 3], [0, 2, 2, 4], [0, 3, 2, 4]):
        with pytest.raises(ValueError):
            plan_calls([True] * 4, cuts, [])
    with pytest.raises(ValueError):
        plan_calls([True] * 4, [0, 4], [4])
