"""The sort key at its edges, on the CPU: the model (tests/model, built from the headers the kernels
use) against the oracle's literal restatement on the pools of tests/key_edge_cases.py — adjacent
fractions with denominators next to 2^cap_bits, equal fractions on several servants, growing
capacities, tier crossings — at every key format: 32-bit divide (cap_bits <= 10), the 64-bit
direct form of the bin boundaries (11), 32-bit radix keys (12 .. 15), 64-bit radix keys
(16 .. 21) and the reference's double (22, 27). Placement, utilisation doubles and running_tasks
must be EQUAL. Plus: the oracle's double pinned to the rationals where the design says both
agree, the verbatim reference class on the widest pools where it is built, and the closed forms
(first_slot_not_below*, servant_slots_before) on thresholds that ARE keys of slots."""
import heapq
from fractions import Fraction

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import key_edge_cases as K
from tests.model import modelbind as M

WIDTHS = (1, 2, 3, 5, 8, 9, 10, 11, 12, 15, 16, 17, 20, 21, 22, 27)
CHUNKS = (0, 64, 1000)


def pool(b, variant, order, near_zero):
    if b == K.FP64_BITS:
        return K.fp64_pool(variant, order)
    return K.edge_pool(b, variant, order, near_zero=near_zero)


def batches(b, sv, variant, seed):
    """(name, requests): plain; with an unknown digest; pools without near-zero servants are
    smaller than their batch (Timeout tail)."""
    yield "plain", K.edge_tasks(sv, variant, seed=seed)
    yield "unknown", K.edge_tasks(sv, variant, seed=seed + 1, unknown=True, own_frac=0.0)


def check(sv, tk, b, variant, chunks=CHUNKS):
    want, wutil, wrun = O.dispatch(sv, tk, "scan")
    for fp64 in (False, True) if b <= K.MAX_EXACT_BITS else (False,):
        for chunk in chunks:
            got, gutil, grun, st = M.dispatch(sv, tk, chunk, fp64)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (b, variant, chunk, fp64, bad[:5], got[bad[:5]], want[bad[:5]])
            assert np.array_equal(gutil, wutil) and np.array_equal(grun, wrun), (b, variant, chunk, fp64)
            assert st.key_bits == (64 if fp64 else K.expected_key_bits(b, variant)), (b, variant, st.key_bits)
    return want


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("b", WIDTHS)
def test_model_matches_oracle_on_edge_pools(b, variant, order):
    for near_zero in (True, False) if b <= K.MAX_EXACT_BITS else (False,):
        sv = pool(b, variant, order, near_zero)
        for name, tk in batches(b, sv, variant, seed=b):
            want = check(sv, tk, b, variant)
            if not near_zero and variant in ("one", "shared") and b >= 3:
                assert (want == O.IDX_TIMEOUT).sum() >= 100, (b, name)
            if name == "unknown":
                assert (want == O.IDX_ENV_NOT_FOUND).sum() > 0


def exact_order(sv, n):
    """The first n slots by (tier, Fraction(r, cap), servant index): a merge of the servants' own
    ascending slot sequences in Python integers — no double, no key."""
    rows = [dict(nproc=int(sv["num_processors"][s]), load=int(sv["current_load"][s]), mt=int(sv["max_tasks"][s]),
                 run=int(sv["running_tasks"][s]), ded=int(sv["priority"][s]) == 1,
                 low=int(sv["memory_available"][s]) < (10 << 30)) for s in range(len(sv["version"]))]

    def entry(s, r):
        row = rows[s]
        cap = K.py_capacity(row, r)
        if not row["mt"] or r >= cap:
            return None
        return (0 if row["ded"] and 2 * r < row["nproc"] else 1, Fraction(r, cap), s, r)

    heap = [e for e in (entry(s, rows[s]["run"]) for s in range(len(rows))) if e]
    heapq.heapify(heap)
    out = []
    while heap and len(out) < n:
        tier, frac, s, r = heapq.heappop(heap)
        out.append(s)
        nxt = entry(s, r + 1)
        if nxt:
            assert nxt[:2] > (tier, frac), "a servant's slots do not ascend"
            heapq.heappush(heap, nxt)
    return out


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("b", [w for w in WIDTHS if w <= K.MAX_EXACT_BITS])
def test_oracle_double_orders_like_the_rationals(b, order):
    """One class, nobody on a servant's host: the requests take the slots in (tier, r / cap,
    registry index) order. Below 2^21 the design claims that the double the reference divides
    orders like the rational itself; this is the rational, from Python's integers."""
    for near_zero in (True, False):
        sv = K.edge_pool(b, "one", order, near_zero=near_zero)
        tk = K.edge_tasks(sv, "one", seed=50 + b, own_frac=0.0)
        want, _, _ = O.dispatch(sv, tk, "scan")
        n = len(want)
        exact = exact_order(sv, n)
        exact = np.array(exact + [O.IDX_TIMEOUT] * (n - len(exact)), np.uint32)
        assert np.array_equal(want, exact), (b, order, near_zero, np.nonzero(want != exact)[0][:5])


def test_fp64_pool_holds_two_rationals_with_one_double():
    """The pool at 2^27 is there for a pair of slots the double cannot tell apart: the reference's
    tie (first registered wins) is the answer, the rational order is not."""
    c1, c2, pairs = K.fp64_big_pair()
    r1, r2 = pairs[0]
    assert Fraction(r1, c1) != Fraction(r2, c2) and float(r1) / float(c1) == float(r2) / float(c2)
    picked, rational_differs = [], []
    for order in (0, 1):
        sv = K.fp64_pool("one", order)
        tk = K.edge_tasks(sv, "one", seed=27, own_frac=0.0)
        want, wutil, _ = O.dispatch(sv, tk, "scan")
        big = [int(s) for s in np.nonzero(sv["max_tasks"] >= c2)[0]]
        mine = [int(s) for s, u in zip(want, wutil) if s in big and u == float(r1) / float(c1)]
        assert mine == sorted(big), (order, mine)  # registry order, whichever capacity comes first
        picked.append([int(sv["max_tasks"][s]) for s in mine])
        rational_differs.append(exact_order(sv, len(want)) != [int(s) for s in want if s < O.IDX_TIMEOUT])
    assert picked[0] == picked[1][::-1]
    assert sorted(rational_differs) == [False, True]  # (the rational order is right in one registry order only)


@pytest.mark.parametrize("b", [21, 22, 27])
def test_widest_pools_against_the_verbatim_reference(b):
    from oracle import refbind as R
    if not R.available():
        pytest.skip("oracle/_ref is not built on this box")
    for order in (0, 1):
        sv = pool(b, "three", order, near_zero=b <= K.MAX_EXACT_BITS)
        tk = K.edge_tasks(sv, "three", seed=70 + b)
        d = R.RefDispatcher()
        d.load_servants(sv)
        ref_idx, _, _, _ = d.dispatch_batch(tk)
        d.close()
        want, _, _ = O.dispatch(sv, tk, "scan")
        assert np.array_equal(want, ref_idx)
        got, _, _, _ = M.dispatch(sv, tk, 64)
        assert np.array_equal(got, ref_idx)


def test_closed_forms_on_thresholds_that_are_slot_keys():
    """model_check_key_forms: every form against a walk (in C++, from the per-slot keys), and every
    output against the integer references of key_edge_cases.key_form_reference — the fp64 key
    bit for bit against numpy's float64 division."""
    import ctypes as C
    tab = K.key_form_cases(200_000, seed=2)
    out = np.zeros(len(tab), K.FORM_OUT_DTYPE)
    n32 = C.c_uint32(0)
    f = M.lib().model_check_key_forms
    f.restype = C.c_uint32
    bad = f(C.c_void_p(tab.ctypes.data), C.c_uint32(len(tab)), C.c_void_p(out.ctypes.data), C.byref(n32))
    assert bad == 0
    ref, ok32 = K.key_form_reference(tab)
    assert n32.value == int(ok32.sum()) and 3 * n32.value >= len(tab)
    for name in K.FORM_OUT_DTYPE.names:
        diff = np.nonzero(out[name] != ref[name])[0]
        assert diff.size == 0, (name, diff.size, tab[diff[:3]], out[name][diff[:3]], ref[name][diff[:3]])
    # the table reaches what it is for: ties on an earlier servant, every width, both formats
    tie = ref["before_exact"] != ref["first"] - tab["running"]
    assert tie.sum() > 2000 and set(tab["cap_bits"][tie].tolist()) == set(range(1, 22))
    assert (tab["fp64"] == 1).sum() > 20_000
