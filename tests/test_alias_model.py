"""Host aliases on the CPU: the plain reference on address strings (tests/alias_reference.py) against
the verbatim reference class, the C oracle and the model — the restatement of the device's
algorithm (tests/model/model.cpp: model_dispatch_alias) — on every case of tests/alias_cases.py;
and the condition that makes those cases worth running: the aliases decide placements."""
import numpy as np
import pytest

from oracle import oraclebind as O
from oracle import refbind as R
from tests import alias_cases as K
from tests import alias_reference as A
from tests.model import modelbind as M

MADE = [f.__name__ for f in K.MADE]
ALL = MADE + list(K.RANDOM_SPECS) + list(K.ONE_SERVANT_SPECS)
ids = lambda keys: [k if isinstance(k, str) else "random-%d-S%d-N%d" % k for k in keys]
small = lambda c: c.n_requests * c.n_servants <= K.PURE_PYTHON_LIMIT


def test_the_address_comparison():
    """The cases of td_scenarios.address_forms / address_prefix_forms."""
    eq = A.is_network_address_equal
    assert eq(":8335", "") and not eq("nocolon", "") and not eq("nocolon", "nocolon")
    assert eq("[::1]:8335", "[::1]") and eq("[::1]:8335", "[:") and eq("[::1]:8335", "[")
    assert not eq("[::1]:8335", "[::1]:8335") and not eq("[::1]:8335", "::1") and not eq("[::1]:8335", "[::1")
    assert eq("a:b:1", "a") and eq("a:b:1", "a:b") and not eq("a:b:1", "a:") and not eq("a:9", "a:b")
    primary, (aip, asv), rid, names = A.intern(
        ["nocolon", ":8335", "[::1]:8335", "a:b:1", "a:9"], ["", "[::1]:8335", "::1", "[", "a", "nocolon", "zz", "zz"])
    assert primary[1] == names[""] == rid[0] and primary[2] == names["[::1]"] and primary[4] == names["a"] == rid[4]
    assert sorted(zip(aip.tolist(), asv.tolist())) == sorted(
        [(names["[:"], 2), (names["["], 2), (names["a"], 3)])
    owned = set(primary.tolist()) | set(aip.tolist())
    assert rid[3] == names["["] and rid[6] == rid[7]
    assert not {int(rid[1]), int(rid[2]), int(rid[5]), int(rid[6])} & owned  # they match nobody
    assert len({int(primary[0]), int(rid[1]), int(rid[2]), int(rid[5]), int(rid[6])}) == 5


def test_the_list_is_sixty_random_cases_over_every_shape():
    assert len(K.RANDOM_SPECS) == 60 == len(set(K.RANDOM_SPECS))
    assert {(S, N) for _, S, N in K.RANDOM_SPECS} == set(K.SHAPES)
    assert set(K.DIFFER) == set(ids(MADE + list(K.RANDOM_SPECS)))


@pytest.mark.parametrize("key", MADE + list(K.RANDOM_SPECS), ids=ids(MADE + list(K.RANDOM_SPECS)))
def test_the_aliases_decide(key):
    """With the alias pairs stripped the reference answers at least 5 % of the requests differently
    (`single`, `duplicates`: at least one); the count is pinned. The stripped answers are also the C
    oracle's, which knows one host per servant."""
    c = K.get(key)
    with_aliases = K.want(c)[0]
    without = O.dispatch(c.sv, c.tk, "scan")[0]
    if small(c):
        assert np.array_equal(without, A.dispatch(c.locations, c.sv, c.requestors, c.tk,
                                                  same_host=A.is_primary_address)[0])
    differ = int((with_aliases != without).sum())
    print(c, "floor", c.floor, "differ", differ)
    assert differ >= c.floor, (c, differ)
    assert differ == K.DIFFER[c.name], (c, differ)


def test_everybody_meets_the_fallback_and_the_timeout():
    c = K.get("everybody")
    idx = K.want(c)[0]
    assert int((idx == A.IDX_TIMEOUT).sum()) >= 1
    fallbacks = []  # grants of the servant that was `self` at that moment, only it being free
    A.dispatch(c.locations, c.sv, c.requestors, c.tk, fallbacks=fallbacks)
    assert fallbacks and all(A.is_network_address_equal(c.locations[idx[t]], c.requestors[t]) for t in fallbacks)
    assert any(c.requestors[t] == "[" for t in fallbacks), fallbacks


# Beyond the pure-Python limit the reference class itself is the reference (K.want); `huge` starts
# from six million running tasks, which the reference class could only be given one grant at a time.
VERBATIM = [k for k in ALL if (k[1] * k[2] <= K.PURE_PYTHON_LIMIT if isinstance(k, tuple)
                               else k not in ("many_classes", "huge"))]


@pytest.mark.skipif(not R.available(), reason="the verbatim reference is not built")
@pytest.mark.parametrize("key", VERBATIM, ids=ids(VERBATIM))
def test_plain_reference_equals_the_reference_class(key):
    c = K.get(key)
    assert small(c)
    want, _, wrun = A.dispatch(c.locations, c.sv, c.requestors, c.tk)
    got, grun = K.verbatim(c.locations, c.sv, c.requestors, c.tk)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (c, bad[:5], got[bad[:5]], want[bad[:5]], [c.requestors[t] for t in bad[:5]])
    assert np.array_equal(grun, wrun), c


@pytest.mark.parametrize("chunk", [64, 256])
@pytest.mark.parametrize("key", ALL, ids=ids(ALL))
def test_model_equals_the_reference(key, chunk):
    """The device's algorithm, replayed on the CPU with the alias pairs in its lookup table."""
    c = K.get(key)
    want, wutil, wrun = K.want(c)
    got, gutil, grun, st = M.dispatch(c.sv, c.tk, chunk_size=chunk, aliases=c.aliases)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (c, bad[:5], got[bad[:5]], want[bad[:5]], [c.requestors[t] for t in bad[:5]])
    assert np.array_equal(gutil, wutil) and np.array_equal(grun, wrun), c


def test_utilisations_follow_from_the_placement():
    for key in ("bracket", "huge", "chain"):
        c = K.get(key)
        idx, util, _ = A.dispatch(c.locations, c.sv, c.requestors, c.tk)
        assert np.array_equal(K.utilisations(c.sv, idx), util)


def test_without_aliases_the_plain_reference_is_the_oracle():
    """Random pools whose locations have one ':' each: no alias pair, and the C oracle's one host
    per servant says it all."""
    seen = 0
    for seed in range(40):
        rng = np.random.default_rng(5000 + seed)
        S, N = int(rng.choice([1, 3, 40])), int(rng.choice([1, 63, 64, 65, 300]))
        n_envs = int(rng.integers(1, 9))
        cols = K.personalities(S, N, n_envs, seed, bool(rng.integers(2)), bool(rng.integers(2)))
        locs = ["%s:%d" % ("abc"[k % 3] * (1 + k // 3 % 3), 8000 + k // 9) for k in range(S)]
        who = sorted({loc[:i] for loc in locs for i in range(len(loc) + 1)})
        req, env, minv = K._requests(rng, N, who, np.ones(len(who)), n_envs, unknown=0.02)
        c = K.Case("no-alias-%d" % seed, locs, cols, req, env, minv)
        assert len(c.aliases[0]) == 0
        want = O.dispatch(c.sv, c.tk, "scan")
        got = A.dispatch(c.locations, c.sv, c.requestors, c.tk)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), c
        seen += int((want[0] < A.IDX_ENV_NOT_FOUND).any())
    assert seen >= 30
