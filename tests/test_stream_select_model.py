"""The model of ydc_stream_inspect_select / ydc_stream_inspect_count (tests/stream_select_model.py) on
hand cases with literal vectors, without a GPU: the unattributed rule with the keys 0 and 0xFFFFFFFF,
UNATTRIBUTED beside REQUESTOR, the extremes of expires_before, the cursor, the page concatenation
property, and the two conditions the randomised differential of tests/test_stream_select_gpu.py puts on
its own inputs."""
import numpy as np
import pytest

from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_select_model as SM
from yadcc_amd import synth

NO_ID, NO_TIME = SM.NO_ID, SM.NO_TIME
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL = 0xFFFFFFFF

# (id, servant, expires_at, zombie, started_at, env_id, requestor_ip, prefetch)
HAND = SM.rows([
    (3, 0, 100, 0, NO_TIME, NO_ID, NO_ID, 0),   # granted while inspection was off
    (4, 1, 50, 1, NO_TIME, NO_ID, NO_ID, 0),    # ... and a zombie
    (7, 0, 100, 0, 10, 0, 0, 0),                # keys 0
    (8, 2, 120, 0, 10, ALL, ALL, 1),            # keys 0xFFFFFFFF: an ordinary digest, an ordinary requestor
    (9, 2, I64_MIN, 1, 11, 0, ALL, 0),
    (12, 1, I64_MAX, 0, 12, 1, 0, 1),
    (1 << 40, 0, 100, 0, I64_MAX, 0, 0, 0),
])


def ids(T, cap=100, **f):
    cols, m = SM.select(T, cap, **f)
    assert m >= len(cols["task_id"]) and len(cols["task_id"]) == min(m, cap)
    return cols["task_id"].tolist(), m


def test_the_empty_filter_and_the_cap():
    assert ids(HAND) == ([3, 4, 7, 8, 9, 12, 1 << 40], 7)
    assert ids(HAND, cap=0) == ([], 7)
    assert ids(HAND, cap=3) == ([3, 4, 7], 7)
    assert ids(HAND, cap=7) == ids(HAND, cap=8)
    cols, _ = SM.select(HAND, 2)
    assert cols["servant_idx"].tolist() == [0, 1] and cols["started_at"].tolist() == [NO_TIME, NO_TIME]
    assert [cols[k].dtype for k in SM.COLS] == list(SM.DTYPES)


def test_the_unattributed_rule_with_the_keys_0_and_all_ones():
    assert ids(HAND, requestor_ip=ALL) == ([8, 9], 2)      # not 3 and 4, whose record says 0xFFFFFFFF too
    assert ids(HAND, env_id=ALL) == ([8], 1)
    assert ids(HAND, requestor_ip=0) == ([7, 12, 1 << 40], 3)
    assert ids(HAND, env_id=0) == ([7, 9, 1 << 40], 3)
    assert ids(HAND, prefetch=0) == ([7, 9, 1 << 40], 3)   # an unattributed lease's 0 says nothing
    assert ids(HAND, prefetch=1) == ([8, 12], 2)
    assert ids(HAND, started_before=I64_MAX) == ([7, 8, 9, 12], 4)  # NO_TIME < anything, and still no match
    assert ids(HAND, started_before=11) == ([7, 8], 2)
    assert ids(HAND, started_before=I64_MIN) == ([], 0)
    assert ids(HAND, unattributed=True) == ([3, 4], 2)
    assert ids(HAND, unattributed=True, zombie=1) == ([4], 1)


def test_unattributed_beside_a_record_predicate_matches_nothing():
    for f in ({"requestor_ip": ALL}, {"requestor_ip": 0}, {"env_id": ALL}, {"prefetch": 0}, {"started_before": I64_MAX}):
        assert ids(HAND, unattributed=True, **f) == ([], 0), f
    assert SM.count(HAND, [{"unattributed": True, "requestor_ip": ALL}, {"unattributed": True}]).tolist() == [0, 2]


def test_the_extremes_of_expires_before():
    assert ids(HAND, expires_before=I64_MIN) == ([], 0)
    assert ids(HAND, expires_before=I64_MIN + 1) == ([9], 1)
    assert ids(HAND, expires_before=I64_MAX) == ([3, 4, 7, 8, 9, 1 << 40], 6)  # strictly before: not lease 12
    assert ids(HAND, expires_before=100) == ([4, 9], 2)
    assert ids(HAND, expires_before=101, servant=0) == ([3, 7, 1 << 40], 3)


def test_table_predicates_and_conjunctions():
    assert ids(HAND, servant=2) == ([8, 9], 2)
    assert ids(HAND, servant=77) == ([], 0)
    assert ids(HAND, zombie=1) == ([4, 9], 2)
    assert ids(HAND, zombie=0, servant=0, requestor_ip=0) == ([7, 1 << 40], 2)
    assert ids(HAND, after_id=0) == ids(HAND)
    assert ids(HAND, after_id=3) == ([4, 7, 8, 9, 12, 1 << 40], 6)
    assert ids(HAND, after_id=12) == ([1 << 40], 1)
    assert ids(HAND, after_id=1 << 40) == ([], 0)
    assert ids(HAND, after_id=(1 << 64) - 1) == ([], 0)
    assert SM.count(HAND, []).tolist() == [] and SM.count(HAND, [{}]).tolist() == [7]


@pytest.mark.parametrize("page", [1, 7, 64, 1000])
def test_pages_concatenated_are_the_filtered_table(page):
    rng = np.random.default_rng(page)
    n = 300
    tid = np.sort(rng.choice(np.arange(1, 5000), n, replace=False)).astype(np.uint64)
    started = np.where(rng.random(n) < 0.5, NO_TIME, rng.integers(0, 50, n))
    T = {"task_id": tid, "servant_idx": rng.integers(0, 4, n).astype(np.uint32),
         "expires_at": rng.integers(0, 100, n).astype(np.int64), "zombie": rng.integers(0, 2, n).astype(np.uint8),
         "started_at": started.astype(np.int64),
         "env_id": np.where(started == NO_TIME, NO_ID, rng.integers(0, 3, n)).astype(np.uint32),
         "requestor_ip": np.where(started == NO_TIME, NO_ID, rng.integers(0, 5, n)).astype(np.uint32),
         "prefetch": np.where(started == NO_TIME, 0, rng.integers(0, 2, n)).astype(np.uint8)}
    for f in ({}, {"servant": 1}, {"requestor_ip": 2, "zombie": 0}, {"unattributed": True}, {"servant": 99},
              {"after_id": int(tid[40]), "env_id": 1}):
        whole, m = SM.select(T, n, **f)
        pgs = SM.pages(T, page, **dict(f))
        assert all(0 < len(p["task_id"]) <= page for p in pgs)
        assert len(pgs) == -(-m // page)
        SM.same(SM.concat(pgs), whole, "pages of %d, %r" % (page, f))


def differential_filters(ws, inspect, rng, now, k=5, caps=(1, 7, 64)):
    """What the randomised differential asks between two ticks: k (cap, filter) pairs drawn from T."""
    T = SM.table(ws, inspect)
    return T, [(int(rng.choice(caps)), SM.random_filter(T, rng, now)) for _ in range(k)]


def test_the_differentials_generator_meets_its_own_conditions():
    """60 ticks of the leased model with inspection: at least 90 % of the random filters match a lease
    and at least 30 % match more than their cap — a condition on the inputs, met by the model alone."""
    sv = synth.make_servants(96, n_tasks_hint=5200 // 2, n_envs=2, seed=5)
    ws = L.LeaseStream(sv, 1500, 1300, 120, L.LeaseTable(), n_envs=2, report_frac=0.3)
    ws.es.hb = 24
    I = IM.attach(ws)
    rng = np.random.default_rng(11)
    asked = some = over = 0
    for _ in range(60):
        ev = ws.next_tick()
        IM.model_tick(L, ws, ev)
        T, qs = differential_filters(ws, I, rng, int(ev["now"]))
        for cap, f in qs:
            _, m = SM.select(T, cap, **f)
            asked, some, over = asked + 1, some + (m >= 1), over + (m > cap)
    assert asked == 300 and some >= 0.9 * asked and over >= 0.3 * asked, (asked, some, over)
