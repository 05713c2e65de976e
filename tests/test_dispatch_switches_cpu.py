"""What each set of dispatch switches changes, pinned on the host, and the planted error the GPU test exists for.

tests/test_gpu_dispatch_switches.py runs the executors with the fallback kernels of conv_plan.cpp's nine switches (and
SISIC_WINOGRAD).  That run is only worth something if every set really moves convolutions to other kernels, so this file pins,
with no device:

  * the multiset of (default plan -> fallback plan) transitions of every set over 171 convolutions (switch_exec.TRANSITIONS: the
    reference architecture at 2x64x64, 2x32x32, 1x72x40 and 64x64x64, and the classifier at 2x224x224), in a fresh process per set
    as in test_conv_plan_cpu.py -- the switches are read once per process;
  * that SISIC_POINTWISE=0 alone changes nothing;
  * that the sets together reach every kernel family and every form of the bf16x3 pointwise kernel at the shapes the workload runs:
    an edit of conv_plan.cpp that makes a set vacuous fails here;
  * that the failure the GPU test is there for -- a GroupNorm applied with the (mean, variance) of the tensor the previous GroupNorm
    read, which is what a stale (scale, shift) pair is -- moves the prediction by at least 100 x PRED_TOL whichever of the 50
    GroupNorms is hit (measured: 7.1e-3 .. 0.96, 142 x .. 19 000 x).
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import arch_ref          # noqa: E402
import switch_exec as sx  # noqa: E402

PRED_TOL = 5e-5          # tests/test_gpu_train.py (a GPU module: not imported where there is no GPU)


def child_record(env):
    out = subprocess.run([sys.executable, os.path.abspath(sx.__file__), "--plans"], env=env, check=True, capture_output=True, text=True)
    return json.loads(out.stdout)


@pytest.fixture(scope="module")
def default_record():
    return child_record(sx.set_env(None))


@pytest.fixture(scope="module")
def records(default_record):
    return {name: child_record(sx.set_env(name)) for name in sx.SETS}


def test_the_walk_is_the_one_the_table_was_counted_over(default_record):
    assert list(default_record) == [f"{B}x{H}x{W}" for B, H, W in sx.RECORD_SHAPES] + ["classifier"]
    distinct = {k: len({w for w, _ in default_record[k]}) for k in sx.table_keys()}
    assert distinct == {"2x64x64": 40, "2x32x32": 40, "1x72x40": 40, "64x64x64": 40, "classifier": 11} and sum(distinct.values()) == 171
    assert all(len(default_record[f"{B}x{H}x{W}"]) == 78 for B, H, W in sx.RECORD_SHAPES)
    assert not any("REFUSED" in p for rows in default_record.values() for _, p in rows)


def test_the_table_has_the_stated_totals():
    assert sx.TABLE_TOTALS == {"wino_bf16x3": 68, "wino_bf16x3+col": 78, "wino_bf16x3+wide": 78, "ksplit": 13, "pointwise_bf16x3": 41,
                               "pointwise_bf16x3+pointwise": 41, "pointwise_ksplit": 18, "s2_bf16x3": 15, "pointwise_staged_ksplit": 4}
    for name, total in sx.TABLE_TOTALS.items():
        assert sum(sx.TRANSITIONS[name].values()) == total, name
    assert sx.TRANSITIONS["winograd"] == {} and list(sx.TRANSITIONS) == list(sx.SETS) == list(sx.RECORD_TOTALS)
    assert [len(v) for v in sx.SETS.values()] == [1, 2, 2, 1, 1, 2, 1, 1, 1, 1, 10]


@pytest.mark.parametrize("name", list(sx.SETS))
def test_transitions_of_a_set(default_record, records, name):
    rec = records[name]
    assert not any("REFUSED" in p for rows in rec.values() for _, p in rows)
    got = sx.transitions(default_record, rec, sx.table_keys())
    assert dict(got) == sx.TRANSITIONS[name], f"{name}: {sorted((got - sx.Counter(sx.TRANSITIONS[name])).items())} appeared, " \
                                              f"{sorted((sx.Counter(sx.TRANSITIONS[name]) - got).items())} are gone"
    assert sum(sx.transitions(default_record, rec).values()) == sx.RECORD_TOTALS[name]
    if name == sx.STAGED_SET:           # only the batch of 64 offers the staged K-split form its 256 workgroups
        assert all(rec[k] == default_record[k] for k in rec if k != "64x64x64")


def test_pointwise_alone_changes_nothing(default_record):
    env = sx.set_env(None)
    env["SISIC_POINTWISE"] = "0"
    assert child_record(env) == default_record


def test_wide_and_col_alone_change_only_what_bf16x3_leaves(default_record):
    for var in ("SISIC_WINO_WIDE", "SISIC_WINO_COL"):
        env = sx.set_env(None)
        env[var] = "0"
        got = sx.transitions(default_record, child_record(env), sx.table_keys())
        assert sum(got.values()) == 10 and all(k.startswith("Winograd third") for k in got), (var, got)


def test_the_sets_together_reach_every_kernel_and_form(default_record, records):
    import arch_plan_table as apt
    reached = {p for rec in [default_record] + list(records.values()) for rows in rec.values() for _, p in rows}
    for kernel in apt.KERNELS:
        assert any(p.startswith(kernel + ",") or p.startswith(kernel + " (") for p in reached), f"no set reaches the {kernel} kernel"
    for form in apt.PWB_FORMS:
        assert any(p.startswith(f"pointwise bf16x3 ({form})") for p in reached), f"no set reaches the {form} form"
    # and each fallback is reached by a set, not by the default
    default = {p for rows in default_record.values() for _, p in rows}
    assert not any(p.startswith(("pointwise f32", "Winograd second")) for p in default)
    assert reached - default >= {"pointwise f32, cfg 20", "Winograd second, cfg 68", "Winograd second, cfg 69", "Winograd second, cfg 91",
                                 "Winograd third, cfg 91", "direct, cfg 11", "direct, cfg 12", "direct, cfg 18"}, sorted(reached - default)


# ---------------------------------------------------------------- the planted error
def forward_with_stale_groupnorm(cfg, sd, x, t, victim):
    """arch_ref.unet_forward with GroupNorm number ``victim`` (in execution order, from 0) normalising by the per-(image, group)
    mean and variance of the tensor the GroupNorm before it read -- a (scale, shift) pair nobody finalised again.  victim None: every
    GroupNorm by its own statistics, through the same written-out arithmetic."""
    state = {"n": 0, "prev": None}

    def group_norm(cfg_, h, w, b, silu):
        B, C = h.shape[:2]
        hg = h.reshape(B, cfg_.norm_num_groups, -1)
        own = (hg.mean(-1, keepdim=True), hg.var(-1, unbiased=False, keepdim=True))
        i, stale = state["n"], state["prev"]
        state["n"], state["prev"] = i + 1, own
        mean, var = stale if i == victim else own
        y = ((hg - mean) * torch.rsqrt(var + cfg_.norm_eps)).reshape(h.shape)
        shape = (1, C) + (1,) * (h.dim() - 2)
        y = y * w.reshape(shape) + b.reshape(shape)
        return F.silu(y) if silu else y

    real, arch_ref.group_norm = arch_ref.group_norm, group_norm
    try:
        with torch.no_grad():
            return arch_ref.unet_forward(cfg, sd, x, t), state["n"]
    finally:
        arch_ref.group_norm = real


def test_a_stale_groupnorm_pair_is_far_over_the_prediction_bar():
    from synt_isic_amd.arch import UNetConfig
    from synt_isic_amd.weights import synthetic_unet_state_dict
    cfg = UNetConfig()
    sd = {k: v.double() for k, v in synthetic_unet_state_dict().items()}
    images, noise, timesteps = sx.unet_inputs()["train64"]
    from oracle import ddpm as oddpm
    x = oddpm.DDPMSchedulerOracle().add_noise(images, noise, timesteps).double()
    with torch.no_grad():
        clean = arch_ref.unet_forward(cfg, sd, x, timesteps)
    same, n = forward_with_stale_groupnorm(cfg, sd, x, timesteps, None)
    assert n == 51 and (same - clean).abs().max().item() <= 1e-12       # the written-out GroupNorm is the GroupNorm
    moved = []
    for victim in range(1, n):
        y, _ = forward_with_stale_groupnorm(cfg, sd, x, timesteps, victim)
        moved.append((y - clean).abs().max().item())
    print(f"stale GroupNorm, 50 victims: the prediction moves by {min(moved):.3e} .. {max(moved):.3e} = {min(moved) / PRED_TOL:.0f} x .. "
          f"{max(moved) / PRED_TOL:.0f} x PRED_TOL")
    assert len(moved) == 50 and min(moved) >= 100 * PRED_TOL, sorted(zip(moved, range(1, n)))[:5]
