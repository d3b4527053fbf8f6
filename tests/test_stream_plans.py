"""CPU tests: the step plans of tests/streamplans.py hold what tests/test_gpu_stream_handover.py relies on -- for every stream
family each order of a small and a large step with a partial block pending and with none, a bulk call exactly at every crossover,
one block below it and one block above it, and no plan beyond 256 KiB.  A plan (or the model of the Step functions) that silently
loses a class fails here, without a GPU."""
import pytest

import streamplans as SP

ORDERS = (("S", "L"), ("L", "S"), ("L", "L"))


def _kinds(family):
    return sorted({SP.bulk_kind(family, op) for ops in SP.plans(family).values() for op, _ in ops if op not in "GV"})


def test_thresholds_are_the_ones_of_the_library():
    """the constants against the text of host_wanted() (bee2_amd/csrc/staging.hpp): a changed crossover must change the plans"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bee2_amd", "csrc", "staging.hpp")).read()
    body = src[src.index("static bool host_wanted("):src.index("static thread_local bool t_dev_seen")]
    assert f"case K_PRIM: return bytes <= {SP.PRIM_HOST_MAX};" in body
    assert f"case K_PARALLEL: return bytes < {SP.PARALLEL_GPU_MIN};" in body
    assert f"case K_POLY: return bytes <= (hostp::gf_have_clmul() ? (size_t){SP.POLY_HOST_MAX_CLMUL} : (size_t){SP.POLY_HOST_MAX_TABLE});" in body
    assert "enum { K_PRIM = 0, K_PARALLEL = 1, K_SERIAL = 2, K_POLY = 3," in src
    assert (SP.K_PRIM, SP.K_PARALLEL, SP.K_SERIAL, SP.K_POLY) == (0, 1, 2, 3)
    for clmul in (True, False):
        top = SP.POLY_HOST_MAX_CLMUL if clmul else SP.POLY_HOST_MAX_TABLE
        assert SP.host_in_auto(SP.K_PARALLEL, 8191, clmul) and not SP.host_in_auto(SP.K_PARALLEL, 8192, clmul)
        assert SP.host_in_auto(SP.K_POLY, top, clmul) and not SP.host_in_auto(SP.K_POLY, top + 16, clmul)
        assert SP.host_in_auto(SP.K_PRIM, 1024, clmul) and SP.host_in_auto(SP.K_SERIAL, 1 << 30, clmul)


def test_length_sets_straddle_every_crossover():
    assert set(SP.PARALLEL_LENGTHS) == {1, 15, 16, 17, 8176, 8191, 8192, 8193, 8208, 20000}
    assert {16, 4096, 4112, 32768, 32784, 70000} <= set(SP.POLY_LENGTHS)
    for kind, lengths in ((SP.K_PARALLEL, SP.PARALLEL_LENGTHS), (SP.K_POLY, SP.POLY_LENGTHS)):
        for t in SP.THRESHOLDS[kind]:
            assert {t - 16, t, t + 16} <= set(lengths)
    assert all(0 < n < 16 for n in SP.SUB_BLOCK)


@pytest.mark.parametrize("family", SP.FAMILIES)
def test_no_plan_exceeds_256_KiB_and_every_op_is_one_the_family_has(family):
    letters = {"CTR": "E", "DWP": "IEADGV", "CHE": "IEADGV", "MAC": "AGV", "HASH": "HG"}.get(family, family[-1] if family in SP.NO_PENDING_FIELD else "HG")
    for name, ops in SP.plans(family).items():
        assert 0 < SP.total_bytes(ops) <= SP.MAX_PLAN_BYTES == 256 * 1024, (family, name)
        assert all(op in letters and (n > 0) == (op not in "GV") for op, n in ops), (family, name)
        if family in SP.NO_PENDING_FIELD:                    # whole blocks; a stealing tail only in the last step, behind a whole block
            assert all(n % 16 == 0 for _, n in ops[:-1]) and (ops[-1][1] % 16 == 0 or ops[-1][1] > 16), (family, name)
        steps = SP.simulate(family, ops)
        assert [(s.op, s.n) for s in steps] == list(ops)
        assert all(0 <= s.pending_before < 192 and 0 <= s.pending_after < 192 for s in steps)


@pytest.mark.parametrize("family", SP.FAMILIES)
def test_every_order_of_small_and_large_steps_with_and_without_a_partial_block(family):
    """small -> large, large -> small, large -> large, for each size-dependent kind of the family, whichever way the polynomial
    crossover falls on the host that runs the GPU test"""
    for clmul in (True, False):
        have = set()
        for ops in SP.plans(family).values():
            have |= SP.orders(family, ops, clmul)
        for kind in _kinds(family):
            for a, b in ORDERS:
                assert (kind, a, b, False) in have, (family, clmul, kind, a, b, "none pending")
                if family not in SP.NO_PENDING_FIELD:
                    assert (kind, a, b, True) in have, (family, clmul, kind, a, b, "partial block pending")
    if family in SP.NO_PENDING_FIELD:
        assert all(s.pending_before == s.pending_after == 0 for ops in SP.plans(family).values() for s in SP.simulate(family, ops))


@pytest.mark.parametrize("family", SP.CROSSOVER_FAMILIES)
def test_every_threshold_has_a_call_at_it_one_block_below_and_one_block_above(family):
    sizes = {}
    for ops in SP.plans(family).values():
        for k, v in SP.bulk_sizes(family, ops).items():
            sizes.setdefault(k, set()).update(v)
    for kind in _kinds(family):
        for t in SP.THRESHOLDS[kind]:
            assert {t - 16, t, t + 16} <= sizes[kind], (family, kind, t)
        # ... and both engines are predicted for it, in either case of the host
        for clmul in (True, False):
            assert {SP.host_in_auto(kind, b, clmul) for b in sizes[kind]} == {True, False}
    # the lengths the plans are drawn from all occur as steps
    lengths = {n for ops in SP.plans(family).values() for _, n in ops}
    want = set(SP.PARALLEL_LENGTHS) if family in ("CTR", "DWP", "CHE") else {n for n in SP.PARALLEL_LENGTHS if n % 16 == 0}
    if family in ("DWP", "CHE"):
        want |= set(SP.POLY_LENGTHS)
    assert want <= lengths, (family, sorted(want - lengths))


@pytest.mark.parametrize("family", ("CTR", "DWP", "CHE"))
def test_sub_block_steps_surround_the_large_ones(family):
    """reserved / filled non-zero before a large step and after one, for each kind"""
    for kind in _kinds(family):
        before = after = False
        for ops in SP.plans(family).values():
            for s in SP.simulate(family, ops):
                if s.op not in "GV" and SP.bulk_kind(family, s.op) == kind and SP.is_large(family, s, True):
                    before |= s.pending_before != 0
                    after |= s.pending_after != 0
        assert before and after, (family, kind)


def test_the_model_counts_the_calls_of_a_step():
    """spot checks of simulate() against the entry points read by hand (capi_belt.hip, capi_bash.hip)"""
    P, S, Y, R = SP.K_PARALLEL, SP.K_SERIAL, SP.K_POLY, SP.K_PRIM
    calls = lambda fam, ops: [s.calls for s in SP.simulate(fam, ops)]      # noqa: E731
    # CTR: leftover gamma first, the rest in ONE call; nothing when the leftover serves the whole step
    assert calls("CTR", [("E", 5), ("E", 8203), ("E", 21), ("E", 3)]) == [((P, 5),), ((P, 8192),), ((P, 21),), ()]
    # CHE: whole blocks in one call, the partial block is one block encryption
    assert calls("CHE", [("E", 5), ("E", 8203), ("E", 8200)]) == [((R, 16),), ((P, 8192),), ((P, 8192), (R, 16))]
    # DWP: the buffered block alone, then the whole blocks; StepA pads the open data first; a tag = one product call + E_K
    assert calls("DWP", [("I", 5), ("I", 4123), ("I", 7), ("A", 40), ("G", 0)]) == \
        [(), ((Y, 16), (Y, 4112)), (), ((Y, 7), (Y, 32)), ((Y, 32), (R, 16))]
    assert calls("CBC-D", [("D", 8192), ("D", 8215)]) == [((P, 8192),), ((P, 8192), (R, 16), (R, 16))]
    assert calls("ECB-E", [("E", 8215)]) == [((P, 8208), (R, 16))]
    assert calls("MAC", [("A", 16), ("A", 1), ("A", 15), ("G", 0)]) == [(), ((S, 1),), (), ((S, 0),)]
    assert calls("HASH", [("H", 31), ("H", 1), ("H", 65), ("G", 0)]) == [(), ((S, 32),), ((S, 64),), ((S, 32),)]
    assert calls("BASH256", [("H", 63), ("H", 1), ("H", 64), ("G", 0)]) == [(), ((S, 1),), ((S, 64),), ((R, 192),)]
    assert [s.pending_after for s in SP.simulate("BASH80", [("H", 151), ("H", 2)])] == [151, 1]
    assert SP.predicted_counts(SP.simulate("DWP", [("I", 32784)])[0], True) == (0, 1)
    assert SP.predicted_counts(SP.simulate("DWP", [("I", 32768)])[0], True) == (1, 0)
    assert SP.predicted_counts(SP.simulate("DWP", [("I", 4112)])[0], False) == (0, 1)


def test_patterns_alternate():
    assert SP.pattern("gc", 5) == "gcgcg" and SP.pattern("cg", 4) == "cgcg"
    r = SP.pattern("random", 40, 3)
    assert len(r) == 40 and set(r) == {"g", "c"} and r == SP.pattern("random", 40, 3) and "gc" in r and "cg" in r


def test_a_plan_that_loses_a_class_is_reported():
    """the check itself: with every step cut to whole blocks the pending plan of CTR has no step inside a gamma block"""
    ops = [(op, n // 16 * 16) for op, n in SP.plans("CTR")["pending"] if n >= 16]
    have = SP.orders("CTR", ops, True)
    assert have and not any(pending for _, _, _, pending in have)
    assert SP.bulk_sizes("CTR", [("E", 5), ("E", 8192)])[SP.K_PARALLEL] == {5, 8181}        # a pending block moves the bulk size
