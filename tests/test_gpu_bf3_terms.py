"""The bf16x3 kernels held to their six-term contract (conv_winograd_bf3.inc:5-17), not to the cross-kernel 1e-5.

Every parity test holds these kernels to 1e-5 * max(1, |ref|) against float64 while their error is 1.5 - 3.6e-7: a kernel that
loses ONE of the six term products in one unrolled body of its channel loop (mid*mid, hi*lo or lo*hi: a wrong operand pairing)
is 2 - 5e-6 away and passes.  Here every case of tests/bf3_ref.py's table runs through ops.conv2d / ops.attention with its
tile_cfg forced and must satisfy

    max |kernel - contract| / top  <=  d_mut / 4

where the contract (the six-term sum in float64, operands placed as the kernel places them) and d_mut (the distance of the
least visible third-order mutant for the SAME inputs) come from the CPU restatement alone.  Runs with one active 8-channel
chunk, walked over the channels, put every body of every pipelined loop under that bound (about 3e-6 of the largest output);
tests/test_bf3_ref_cpu.py proves for the same table that d_mut >= 16 * the fp32 emulation's own distance, so the bound leaves a
correct kernel four times the emulation's room for its summation order and its fp32 Winograd transforms.

SISIC_TEST_ERRLOG: one line per run -- kernel distance, bound, case, d_emul, d_mut."""
import os

import pytest
import torch

import bf3_ref as R
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _kernel(case, t, packed):
    from synt_isic_amd import ops
    if case.kind == "att":
        return ops.attention(_d(t["qkv"]), R.CHUNK)
    gn = t["gn"]
    k = 1 if case.kind == "pw" else 3
    return ops.conv2d(_d(t["x"]), packed[0], case.cout, k, bias=_d(t["bias"]), x2=_d(t["x2"]), stride=2 if case.kind == "s2" else 1,
                      upsample=case.ups, gn_scale=_d(gn[0]) if gn else None, gn_shift=_d(gn[1]) if gn else None,
                      gn_silu=case.pro, tile_cfg=case.cfg, w_winograd=packed[1])


def _pack(case, w):
    from synt_isic_amd import ops
    wd = _d(w)
    second = {"wino": ops.pack_winograd_weight, "s2": ops.pack_conv_s2_weight}.get(case.kind)
    return ops.pack_conv_weight(wd), (second(wd) if second else None)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.ident)
def test_bf16x3_kernel_keeps_all_six_term_products(case):
    packed, failures = None, []
    for chunk in R.runs(case):
        t = R.inputs(case, chunk)
        if case.kind == "att":
            # the form follows the batch (launch_attention; SISIC_ATT_QB is read once per process): the case must select its own
            assert (case.B * (case.cin // R.CHUNK) * ((case.H + 255) // 256) >= 4 * 256) == (case.cfg == 2)
        elif packed is None:
            packed = _pack(case, t["w"])                      # (the weights of a case are the same in all of its runs)
        got = _kernel(case, t, packed).cpu().double()
        ref = R.reference(case, chunk)
        if case.images is not None:
            got = got[list(case.images)]
        assert got.shape == ref.contract.shape
        dist = (got - ref.contract).abs().max().item() / ref.top
        bound = ref.d_mut / R.KERNEL_ROOM
        what = f"{case.ident} chunk {chunk}"
        if os.environ.get("SISIC_TEST_ERRLOG"):
            with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
                f.write(f"{dist:.3e}\t{bound:.3e}\tbf3 terms {what}\td_emul={ref.d_emul:.3e}\td_mut={ref.d_mut:.3e}\n")
        if not (torch.isfinite(got).all() and dist <= bound):
            failures.append(f"{what}: |kernel - contract| / top = {dist:.3e} > d_mut / 4 = {bound:.3e} (d_emul {ref.d_emul:.3e})")
    assert not failures, "\n".join(failures)
