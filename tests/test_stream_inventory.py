"""Every entry point of include/sisic.h that takes a `void* stream` has a case that drives it on a non-default stream
(tests/test_gpu_streams.py), or a stated reason why not.  Runs without a GPU: the registry is plain data in stream_probe.py."""
import os
import re

import stream_probe as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "sisic.h")).read()


def _stream_entry_points():
    """names of the declared functions with a `void* stream` parameter (comments stripped, as tests/test_abi.py does)"""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = []
    for name, params in re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src):
        if re.search(r"\bvoid\s*\*\s*stream\b", params):
            names.append(name)
    return sorted(set(names))


def _covered():
    named = {}
    for case, (entries, _) in sp.CASES.items():
        for e in entries:
            named.setdefault(e, []).append(case)
    for test, entries in sp.OTHER_TESTS.items():
        for e in entries:
            named.setdefault(e, []).append(test)
    return named


def test_every_stream_entry_point_has_a_case():
    entry_points = _stream_entry_points()
    assert len(entry_points) > 50 and "sisic_conv2d" in entry_points and "sisic_sample_frames_edit" in entry_points, entry_points
    named = _covered()
    orphans = [e for e in entry_points if e not in named and e not in sp.EXEMPT]
    assert not orphans, ("entry points with a `void* stream` that no case of tests/stream_probe.py drives on a side stream (add a "
                         f"case, or an exemption with its reason): {orphans}")
    # the registry speaks of the header as it is: no stale names, no exemption of something that has a case or no stream
    declared = set(re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert not sorted(set(named) - declared), sorted(set(named) - declared)
    for e, reason in sp.EXEMPT.items():
        assert e in entry_points and e not in named and reason and "\n" not in reason, e


def test_every_case_has_a_builder_and_every_builder_a_case():
    import test_gpu_streams as t
    assert sorted(t.BUILDERS) == sorted(sp.CASES)
    for name in sp.OTHER_TESTS:
        assert callable(getattr(t, name, None)), name


def test_synchronising_cases_quote_the_header():
    """a case may wait for its stream only where include/sisic.h says the call synchronises, in these words"""
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+/?", " ", _header()).split())
    for name, (_, why) in sp.CASES.items():
        if why is not None:
            assert " ".join(why.split()) in flat, f"{name}: include/sisic.h does not say \"{why}\""
