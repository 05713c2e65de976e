"""Device-noise mode, the part that needs no GPU: the numpy restatement of the contract is the
published Philox4x32-10, the C ABI declares and binds the new entries, and the public interface refuses an unknown mode."""
import os
import re

import numpy as np
import pytest

import philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sisic_noise_fill", "sisic_noise_bits", "sisic_sample_frames_rng")


def test_restatement_reproduces_the_known_answer_vectors():
    """Random123's three published vectors for philox4x32-10, one at a time and as one batch."""
    for ctr, key, want in philox_ref.KAT:
        got = philox_ref.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    same_key = [k for k in philox_ref.KAT if k[1] == (0, 0)]
    got = philox_ref.philox4x32_10(np.array([k[0] for k in same_key], dtype=np.uint32), (0, 0))
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in same_key]


def test_restatement_lays_blocks_out_as_the_contract_says():
    """element e of an image lies in block e >> 2 with counter (e >> 2, step, tag, 0) and key (seed low, seed high); u1 > 0"""
    seed, step, tag = (5 << 32) | 7, 999, 1
    bits = philox_ref.noise_bits(seed, step, tag, 10)
    assert bits.shape == (12,) and bits.dtype == np.uint32
    one = philox_ref.philox4x32_10(np.array([[2, step, tag, 0]], dtype=np.uint32), (7, 5))[0]
    assert (bits[8:12] == one).all()
    z, rad = philox_ref.noise_normals(seed, step, tag, 10)
    assert z.shape == (10,) and np.isfinite(z).all() and (np.abs(z) <= rad + 1e-12).all()
    # the extremes of a word: u1 = 2^-24 (largest radius, finite) and u1 = 1 (radius 0)
    zz, rr = philox_ref.normals_from_bits(np.array([0, 0, 0xFFFFFFFF, 0], dtype=np.uint32))
    assert np.isfinite(zz).all() and abs(rr[0] - np.sqrt(48 * np.log(2.0))) < 1e-12 and rr[2] == 0.0


def test_header_declares_and_binding_table_binds_the_new_entries():
    from synt_isic_amd import _lib
    src = open(os.path.join(ROOT, "include", "sisic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/sisic.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "#define SISIC_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "sisic.h")).read()      # additive only
    # seeds cross the boundary as host uint64, the step offset as an int right behind them
    import ctypes as C
    args = _lib.SIGNATURES["sisic_sample_frames_rng"][1]
    assert args[9] == C.POINTER(C.c_uint64) and args[10] == C.c_int and len(args) == len(_lib.SIGNATURES["sisic_sample_frames"][1]) + 1
    assert _lib.SIGNATURES["sisic_noise_fill"][1][4] == C.POINTER(C.c_uint64)


def test_library_exports_the_new_entries():
    from synt_isic_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name)
    # argument validation needs no GPU
    assert lib.sisic_noise_fill(None, None, 1, 4, None, 0, 0, None) == _lib.SISIC_EINVAL
    assert lib.sisic_sample_frames_rng(None, None, 1, 32, 32, 4, None, None, 1.0, None, 0, None, None, None, None, None,
                                       None) == _lib.SISIC_EINVAL
    assert b"seeds" in lib.sisic_last_error()


def test_unknown_noise_mode_is_refused_before_the_gpu_is_touched():
    """no model is loaded and this machine may have no GPU: the ValueError has to come first"""
    from synt_isic_amd import sampler as S
    s = S.Sampler("cuda")
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="noise must be one of"):
            s.generate_seeds("NV", [0], T=4, size=(32, 32), noise=bad)
        with pytest.raises(ValueError, match="noise must be one of"):
            s.generate(0, "NV", 4, size=(32, 32), noise=bad)
        with pytest.raises(ValueError, match="noise must be one of"):
            s.generate_images("NV", [0], 4, size=(32, 32), noise=bad)
    with pytest.raises(KeyError):                       # a known mode goes on to the model lookup
        s.generate_seeds("NV", [0], T=4, size=(32, 32), noise="device")
    with pytest.raises(ValueError):
        S.DeviceNoise((-1,))
    assert S.DeviceNoise([3, 2 ** 40]).seeds == (3, 2 ** 40) and S.DeviceNoise([1]).step0 == 0
