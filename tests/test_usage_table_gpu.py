"""The usage table (stream_usage.h: k_usage_accrue, k_usage_find, k_usage_fold, k_usage_load,
k_usage_rehash) where its suite's sequential requestor ids never take it: along chains of ids that share
a home slot (across the wrap, touching, through a growth, across the fold's tile boundary), with rows of
W whose counts need the upper half of wave_sum_wide, over lease tables whose every lease lies in a slot
the test chose (one thread's four slots, one wave, the four waves' leads, two workgroups), and at the two
places where the host's bound on the keys is bumped outside a tick.

Every expectation is tests/usage_table_cases.py's Expect: plain Python integers from the crafted list
itself, never the library's answer; get and find are compared with it integer for integer after every
tick and load. tests/test_usage_table_model.py rehearses every input on the CPU. No test asserts a time.

Where the leases lie: a lease table restored from ids computed to be alone in their home slot
(tests/lease_table_cases.py: slot == home, displacement 0) holds them there by the table's own rule.
No call of the library promises to list L in slot order (ydc_stream_inspect_tasks, ydc_stream_leases_get
and the select sort by id on their way out), so that order cannot be shown from outside; the evidence
that the patterns reach the threads they name is that library builds with the thread merge, the lead
merge or its clearing broken, which differ only at those slots, fail these tests."""
import numpy as np
import pytest

from tests import hash_index_cases as H
from tests import lease_table_cases as LT
from tests import stream_inspect_model as IM
from tests import stream_usage_model as U
from tests import test_stream_requestor_gpu as RQ
from tests import usage_table_cases as UC
from tests.usage_table_cases import BITS, SIZE
from yadcc_amd import binding, snapshot, streaming

pytestmark = pytest.mark.gpu
WAITING = RQ.WAITING
ENDS = [0, 0xFFFFFFFF]
COMBINE = pytest.mark.parametrize("combine", [None, "0"], ids=["combined", "per lane"])


def _combine(monkeypatch, combine):
    if combine is not None:
        monkeypatch.setenv("YDC_REQUESTOR_COMBINE", combine)


def same(ctx, exp, ask=(), what=""):
    """ydc_stream_usage_get and _find against the expectation. -> the totals."""
    got, tot = streaming.usage(ctx)
    want, wtot = exp.get()
    assert len(got) == len(want), "%s: %d rows, expected %d" % (what, len(got), len(want))
    for k in U.DTYPE.names:
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, "%s: get %s: requestor %#x gpu %d expected %d (%d rows differ)" % (
            what, k, int(want["requestor_ip"][bad[0]]), int(got[k][bad[0]]), int(want[k][bad[0]]), bad.size)
    for k, v in wtot.items():
        assert tot[k] == v, "%s: totals %s gpu %d expected %d" % (what, k, tot[k], v)
    s = tot["slots"]
    assert s >= SIZE and s & (s - 1) == 0 and 2 * tot["n_keys"] <= s, tot
    q = np.array(sorted(exp.rows) + [int(x) for x in ask] + ENDS, np.uint64).astype(np.uint32)
    found, model = ctx.stream_usage_find(q), exp.find(q)
    for k in U.DTYPE.names:
        bad = np.nonzero(found[k] != model[k])[0]
        assert bad.size == 0, "%s: find %s: requestor %#x gpu %d expected %d (%d rows differ)" % (
            what, k, int(q[bad[0]]), int(found[k][bad[0]]), int(model[k][bad[0]]), bad.size)
    return tot


def rpc_stream(sv, quantum=1, want=0, max_requests=600, max_rows=1 << 13, max_waiting=1100, max_leases=1 << 14):
    """An rpc stream with inspection and usage on. -> (context, expectation)."""
    ctx = RQ.uploaded(sv)
    ctx.stream_begin_rpc(8, 16, max_requests, max_rows, max_waiting, max_leases, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    ctx.stream_usage_begin(quantum, want)
    return ctx, UC.Expect(quantum)


def requests(ips, first_tag, n_imm=None, n_pre=None):
    ips = np.asarray(ips, np.uint64).astype(np.uint32)
    n = len(ips)
    return {"env_id": np.zeros(n, np.uint32), "min_version": np.zeros(n, np.uint32), "requestor_ip": ips,
            "n_immediate": np.ones(n, np.uint32) if n_imm is None else np.asarray(n_imm, np.uint32),
            "n_prefetch": np.zeros(n, np.uint32) if n_pre is None else np.asarray(n_pre, np.uint32),
            "lease_for": np.full(n, 10 ** 6, np.int64), "deadline": np.full(n, 1 << 40, np.int64),
            "tag": np.arange(first_tag, first_tag + n, dtype=np.uint64)}


def rpc_tick(ctx, exp, now, req, L, W):
    """One tick on both sides. L, W: the test's own lists of what the stream holds in front of the tick."""
    exp.tick(now, L, W)
    return RQ.rpc_tick(ctx, now, req)


def rows_of(req):
    return (req["n_immediate"].astype(np.int64) + req["n_prefetch"]).tolist()


def finish(ctx):
    ctx.stream_end()
    ctx.close()


# ---- A. chains ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", H.HOMES)
def test_load_alone_along_a_chain(h):
    """k_usage_load: a chain's ids in one call in a permuted order, five distinct sums each; a second call
    with every id three times (duplicates race for one claim and add together). find: the members, absent
    ids of the same home, absent ids whose home lies inside the run and behind it, 0 and 0xFFFFFFFF."""
    ctx, exp = rpc_stream(RQ.saturated_registry())
    for n in H.LENGTHS:
        ids = UC.chain(h, n)
        absent = H.absent_around(BITS, h, n, ids, ids=True)
        rows = UC.sums_for(ids, n)
        for rep, batch in ((1, UC.permuted(rows, h + n)), (3, UC.permuted(rows * 3, h + n + 1))):
            ctx.stream_usage_load(UC.as_rows(batch))
            exp.load(batch)
            tot = same(ctx, exp, absent, "home %d, %d ids, each %d times" % (h, n, rep))
            assert tot["n_keys"] == n and tot["slots"] == H.slots_usage(n if rep == 1 else 4 * n)
        got, _ = streaming.usage(ctx, reset=True)
        assert len(got) == n
        exp.reset()
    finish(ctx)


def test_ids_0_and_all_ones_on_chains_holding_leases_and_waiting():
    """0 and 0xFFFFFFFF, each amid 63 ids of its home: loaded, then as holders of leases and as waiting
    requestors in one accrual. 0xFFFFFFFF is an ordinary key: whose time is unattributed is told by
    started_at, not by the id."""
    zero, ones, hf = UC.ends()
    both = zero + ones
    absent = H.absent_around(BITS, 0, 64, zero, ids=True) + H.absent_around(BITS, hf, 64, ones, ids=True)
    ctx, exp = rpc_stream(RQ.roomy_registry(16), quantum=100)  # 128 slots
    batch = UC.permuted(UC.sums_for(both), 3)
    ctx.stream_usage_load(UC.as_rows(batch))
    exp.load(batch)
    same(ctx, exp, absent, "0 and all ones, loaded")
    streaming.usage(ctx, reset=True)
    exp.reset()
    order = UC.permuted(both, 4)
    r = rpc_tick(ctx, exp, 10, requests(order, 1), (), ())
    assert int(r["n_granted"].sum()) == 128 and r["n_waiting"] == 0
    L = [(ip, False, False) for ip in order]
    again = UC.permuted(both, 5)
    req = requests(again, 1000, n_imm=1 + np.arange(128) % 2, n_pre=np.arange(128) % 3)
    r = rpc_tick(ctx, exp, 11, req, L, ())
    assert (r["status"] == WAITING).all() and r["n_waiting"] == 128
    W = list(zip(again, rows_of(req)))
    same(ctx, exp, absent, "inside the first quantum")
    assert not exp.rows
    for now in (100, 350):  # (dq 1: L and W claim the two chains in one launch; dq 2)
        r = rpc_tick(ctx, exp, now, requests([], 5000), L, W)
        assert r["n_waiting"] == 128 and r["n_leases"] == 128
        tot = same(ctx, exp, absent, "0 and all ones, now %d" % now)
        assert tot["unattributed_time"] == 0 and tot["n_keys"] == 128
    assert exp.rows[0][0] == 3 and exp.rows[0xFFFFFFFF][0] == 3 and exp.rows[0][3] == 3
    finish(ctx)


def test_two_chains_whose_runs_touch_across_the_wrap():
    """40 ids of home 1021 go on through slots 0 .. 36 while 40 more have home 0: one run of 80. Loaded in
    three orders, then claimed by the accrual over W."""
    a, b, absent = UC.touching()
    ctx, exp = rpc_stream(RQ.saturated_registry())
    for salt, order in enumerate((a + b, b + a, UC.permuted(a + b, 7))):
        batch = [r for ip in order for r in UC.sums_for([ip], salt)]
        ctx.stream_usage_load(UC.as_rows(batch))
        exp.load(batch)
        assert same(ctx, exp, absent, "touching chains, order %d" % salt)["slots"] == SIZE
        streaming.usage(ctx, reset=True)
        exp.reset()
    order = UC.permuted(a + b, 8)
    req = requests(order, 1, n_pre=np.arange(80) % 4)
    r = rpc_tick(ctx, exp, 10, req, (), ())
    assert (r["status"] == WAITING).all()
    W = list(zip(order, rows_of(req)))
    for now in (11, 14):
        rpc_tick(ctx, exp, now, requests([], 500), (), W)
        assert same(ctx, exp, absent, "touching chains in W, now %d" % now)["n_keys"] == 80
    finish(ctx)


@COMBINE
@pytest.mark.parametrize("h", H.HOMES)
def test_chain_claimed_by_the_accrual_over_the_waiting_queue(h, combine, monkeypatch):
    """W of a saturated rpc stream, where queue position i is lane i % 64: 64 distinct ids of one home fill
    one wave (four combine rounds, then 60 lanes race for one run); after a reset all 257 at once, over five
    waves and two workgroups."""
    _combine(monkeypatch, combine)
    ids = UC.chain(h, 257)
    ctx, exp = rpc_stream(RQ.saturated_registry())
    W, tag = [], 1
    for n, now in ((64, 10), (257, 20)):
        H.one_chain(ids[:n], BITS, h)
        new = UC.permuted(ids[len(W):n], h + n)
        req = requests(new, tag, n_imm=1 + np.arange(len(new)) % 2, n_pre=np.arange(len(new)) % 3)
        tag += len(new)
        r = rpc_tick(ctx, exp, now, req, (), W)
        W += list(zip(new, rows_of(req)))
        assert (r["status"] == WAITING).all() and r["n_waiting"] == n
        streaming.usage(ctx, reset=True)  # (every member is claimed again by the next accrual, in one launch)
        exp.reset()
        absent = H.absent_around(BITS, h, n, ids[:n], ids=True)
        for step in (1, 3):
            r = rpc_tick(ctx, exp, now + step, requests([], 9000), (), W)
            assert r["n_waiting"] == n and r["n_waiting_rows"] == sum(k for _, k in W)
            tot = same(ctx, exp, absent, "home %d, %d in W, now %d" % (h, n, now + step))
            assert tot["n_keys"] == n and tot["slots"] == SIZE
    finish(ctx)


@pytest.mark.parametrize("h", [100, 1021])
def test_chain_claimed_over_leases_and_the_waiting_queue_in_one_launch(h):
    """128 ids of one home hold leases and 200 of that home wait, all met for the first time by one accrual
    (both arrive inside the first quantum): a slot claimed by a workgroup over L is found by one over W, and
    the other way round for those that only wait."""
    ids = UC.chain(h, 200)
    ctx, exp = rpc_stream(RQ.roomy_registry(16), quantum=100)  # 128 slots
    holders = UC.permuted(ids[:128], h)
    r = rpc_tick(ctx, exp, 10, requests(holders, 1), (), ())
    assert int(r["n_granted"].sum()) == 128 and r["n_waiting"] == 0
    L = [(ip, False, False) for ip in holders]
    waiters = UC.permuted(ids, h + 1)
    req = requests(waiters, 1000, n_pre=np.arange(200) % 3)
    r = rpc_tick(ctx, exp, 11, req, L, ())
    assert (r["status"] == WAITING).all() and r["n_waiting"] == 200
    W = list(zip(waiters, rows_of(req)))
    assert H.slots_usage(UC.bound(0, 328, 328)) == SIZE
    absent = H.absent_around(BITS, h, 200, ids, ids=True)
    for now in (100, 250, 300):  # (dq 1, 1, 1)
        rpc_tick(ctx, exp, now, requests([], 5000), L, W)
        tot = same(ctx, exp, absent, "home %d, L and W, now %d" % (h, now))
        assert tot["n_keys"] == 200 and tot["slots"] == SIZE
    assert sum(1 for r in exp.rows.values() if r[0] == 3 and r[3] == 3) == 128 and sum(1 for r in exp.rows.values() if r[0] == 0) == 72
    finish(ctx)


@pytest.mark.parametrize("way", ["begin", "load"])
@pytest.mark.parametrize("kind", ["stay0", "stay1", "split"])
@pytest.mark.parametrize("h", H.HOMES)
def test_growth_with_a_chain_in_the_table(h, kind, way):
    """257 ids of one home at 1024 slots, five distinct sums each; the table doubles, by a begin that asks
    for 600 or by a load of 300 further keys, and the chain stays at h, moves to h + 1024 or splits. Every
    row is carried over column by column; absent ids around both new homes read zeros."""
    ids, homes = UC.doubled(h, kind)
    ctx, exp = rpc_stream(RQ.saturated_registry())
    batch = UC.permuted(UC.sums_for(ids, 1), h)
    ctx.stream_usage_load(UC.as_rows(batch))
    exp.load(batch)
    assert same(ctx, exp, H.absent_around(BITS, h, 257, ids, ids=True), "before the growth")["slots"] == SIZE
    more = UC.further_keys(300, ids)
    if way == "begin":
        ctx.stream_usage_begin(1, 600)
        more = []
    else:
        batch = UC.sums_for(more, 2)
        ctx.stream_usage_load(UC.as_rows(batch))
        exp.load(batch)
    absent = []
    for hh, n in homes.items():
        absent += H.absent_around(BITS + 1, hh, n, ids + more, ids=True)
    tot = same(ctx, exp, absent, "home %d, %s, grown by a %s" % (h, kind, way))
    assert tot["slots"] == 2 * SIZE and tot["n_keys"] == 257 + len(more)
    finish(ctx)


def test_fold_across_tiles_and_the_wrap():
    """2048 slots, three chains of 65: one run crosses the fold's tile boundary 1023 -> 1024, one the wrap,
    one neither. get returns every key exactly once; again after a reset."""
    chains = UC.fold_chains()
    ctx, exp = rpc_stream(RQ.saturated_registry(), want=600)
    everyone = chains[0] + chains[1] + chains[2]
    absent = []
    for c, hh in zip(chains, (1021, 2045, 300)):
        absent += H.absent_around(BITS + 1, hh, 65, c, ids=True)
    for rep in range(2):
        batch = UC.permuted(UC.sums_for(everyone, rep), rep)
        ctx.stream_usage_load(UC.as_rows(batch))
        exp.load(batch)
        tot = same(ctx, exp, absent, "three chains in two tiles, round %d" % rep)
        assert tot["slots"] == 2 * SIZE and tot["n_keys"] == 195
        raw, _ = ctx.stream_usage_get()
        assert sorted(raw["requestor_ip"].tolist()) == sorted(everyone), "a key twice or not at all"
        got, _ = streaming.usage(ctx, reset=True)
        assert len(got) == 195
        exp.reset()
        same(ctx, exp, everyone, "after the reset")
    finish(ctx)


# ---- B. the upper half of wave_sum_wide ---------------------------------------------------------------

@COMBINE
def test_rows_that_need_the_upper_half_of_the_wave_sum(combine, monkeypatch):
    """One wave of W: one requestor's five entries ask for 65535, 65536, 65537, 131071 and 1 rows (the lower
    halves' sum carries past bit 16, the upper halves are not zero), the other 59 entries are a second
    requestor's with one row each. wait_time = k dq entries, wait_row_time = k dq rows, per requestor."""
    _combine(monkeypatch, combine)
    wave = UC.wide_wave()
    ctx, exp = rpc_stream(RQ.saturated_registry(), max_requests=64, max_rows=1 << 19, max_waiting=128, max_leases=1 << 19)
    req = requests([ip for ip, _, _ in wave], 1, n_imm=[a for _, a, _ in wave], n_pre=[b for _, _, b in wave])
    r = rpc_tick(ctx, exp, 10, req, (), ())
    assert (r["status"] == WAITING).all() and r["n_waiting"] == 64 and r["n_waiting_rows"] == 327680 + 59
    W = [(ip, a + b) for ip, a, b in wave]
    for k, now in enumerate((11, 12, 15)):
        r = rpc_tick(ctx, exp, now, requests([], 100), (), W)
        assert r["n_waiting"] == 64 and r["n_waiting_rows"] == 327680 + 59
        same(ctx, exp, (), "the wide wave, now %d" % now)
    assert exp.rows[UC.HEAVY] == [0, 0, 0, 5 * 5, 5 * 327680] and exp.rows[UC.LIGHT] == [0, 0, 0, 5 * 59, 5 * 59]
    finish(ctx)


# ---- C. leases at exact slots -------------------------------------------------------------------------

def play(plan, bits=BITS, ask=()):
    """The plan's lease table restored, its records loaded, usage begun; three ticks (dq 0, 1, 3), the first
    of which turns the leases that expire at 0 into zombies."""
    ls, caps, at = UC.exact_stream(plan, bits)
    ctx = binding.Context(device=0)
    ctx.stream_restore(snapshot.build(LT.state(ls, caps)))
    ctx.stream_inspect_begin(discovered_at=np.zeros(ls.es.n, np.int64))
    ctx.stream_inspect_load(**UC.records(plan, at))
    ctx.stream_usage_begin(1)
    exp = UC.Expect()
    L = UC.triples(plan)
    for now in (1, 2, 5):
        exp.tick(now, L)
        _, n_leases = RQ.leased_tick(ctx, now, [])
        assert n_leases == len(plan), "a lease was swept"
        if now == 1:
            tk = ctx.stream_inspect_tasks()
            by_id = {at[s]: plan[s] for s in plan}
            want = [by_id[int(t)] for t in tk["task_id"]]
            assert tk["zombie"].tolist() == [int(le.zombie) for le in want], "the zombies are not the plan's"
            assert tk["prefetch"].tolist() == [int(le.prefetch and le.ip is not None) for le in want]
            assert [None if a == IM.NO_TIME else int(ip) for a, ip in zip(tk["started_at"].tolist(), tk["requestor_ip"].tolist())] == \
                [le.ip for le in want]
        tot = same(ctx, exp, ask, "now %d" % now)
    assert tot["quanta"] == 4 and tot["unattributed_time"] == 4 * sum(le.ip is None for le in plan.values())
    finish(ctx)
    return exp


@COMBINE
@pytest.mark.parametrize("pattern", UC.THREAD_PATTERNS)
def test_one_threads_four_slots(pattern, combine, monkeypatch):
    """A thread's four slots hold 1 .. 4 requestors in every arrangement, with holes; the zombie and the
    prefetch byte belong to the second or third requestor; the next thread holds a lease without details."""
    _combine(monkeypatch, combine)
    exp = play(UC.thread_plan(pattern))
    assert exp.rows[0][0] == 4 * 2 * (pattern.count("A") + 1) and exp.unattributed == 8


@COMBINE
@pytest.mark.parametrize("ids", ["sequential", "home 1021"])
def test_one_wave_with_a_hot_lead_and_six_second_keys(ids, combine, monkeypatch):
    """Wave 0: every thread's first requestor is the hot one, its second one of six; wave 1: 64 distinct
    first requestors, which with "home 1021" are one chain of the usage table across its wrap."""
    _combine(monkeypatch, combine)
    distinct = UC.chain(1021, 64) if ids == "home 1021" else None
    ask = H.absent_around(BITS, 1021, 64, distinct, ids=True) if distinct else ()
    exp = play(UC.wave_plan(distinct), ask=ask)
    assert exp.rows[UC.HOT] == [4 * 77, 4 * 7, 4 * 8, 0, 0]


@COMBINE
@pytest.mark.parametrize("name", sorted(UC.LEADS))
def test_the_four_waves_leads(name, combine, monkeypatch):
    _combine(monkeypatch, combine)
    keys = UC.LEADS[name]
    exp = play(UC.leads_plan(keys))
    k = sum(x == UC.X for x in keys)
    assert exp.rows[UC.X][0] == 4 * 7 * k and exp.rows[UC.X][2] == 4 * k


@COMBINE
def test_two_workgroups_share_the_hot_key_and_a_key_at_their_seam(combine, monkeypatch):
    _combine(monkeypatch, combine)
    exp = play(UC.two_workgroups_plan(), bits=BITS + 1)
    assert exp.rows[UC.ONLY_AT_THE_SEAM] == [4 * 8, 4, 4, 0, 0] and exp.rows[UC.HOT][0] == 4 * 18


# ---- D. the host's bound -------------------------------------------------------------------------------

def _ramped():
    """A leased stream, usage on its 1024-slot floor with 500 requestors claimed and 600 leases in L, the
    clock at 70 with quantum 10. -> (context, expectation, {lease id: requestor})."""
    ctx = RQ.uploaded(RQ.roomy_registry())
    ctx.stream_begin_leased(8, 16, 600, 2048, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    ctx.stream_usage_begin(10)
    exp, whose, now = UC.Expect(10), {}, 0
    for reqs in UC.ramp() + [[]]:
        now += 10
        exp.tick(now, [(ip, False, False) for ip in whose.values()])
        ids, n_leases = RQ.leased_tick(ctx, now, reqs, lease_for=10 ** 6)
        whose.update(zip([int(t) for t in ids], reqs))
        assert n_leases == len(whose)
        assert same(ctx, exp, (), "the ramp, now %d" % now)["slots"] == SIZE
    assert now == 70 and len(exp.rows) == UC.RAMP_KEYS and len(whose) == UC.RAMP_LEASES
    return ctx, exp, whose


def _after_the_strangers(ctx, exp, L, filed):
    """Two ticks inside the quantum, then the accruing one: the table has grown in front of it, to what the
    bound asks for when each of the `filed` records may name a requestor the table has not met."""
    grown = H.slots_usage(UC.bound(UC.RAMP_KEYS, filed, UC.RAMP_LEASES))
    assert ctx.stream_usage_get()[1]["slots"] == SIZE < grown
    for now in (71, 72):
        exp.tick(now, L)
        RQ.leased_tick(ctx, now, [])
        same(ctx, exp, UC.strangers()[:40], "inside the quantum, now %d" % now)
    assert ctx.stream_usage_get()[1]["slots"] == grown, "the table has not grown in front of the accruing tick"
    for now in (80, 100):
        assert exp.tick(now, L) == (1 if now == 80 else 2)
        RQ.leased_tick(ctx, now, [])
        tot = same(ctx, exp, (), "behind the strangers, now %d" % now)
        assert tot["n_keys"] == UC.RAMP_KEYS + UC.STRANGERS and tot["slots"] == grown
    finish(ctx)


def test_inspect_load_with_usage_on_names_requestors_the_table_has_not_met():
    """ydc_stream_inspect_load rewrites the records of 520 leases to 520 new requestors inside a quantum:
    500 + 520 keys do not fit half of 1024 slots, and only the host's bound knows before the accrual."""
    ctx, exp, whose = _ramped()
    ids, new = sorted(whose)[:UC.STRANGERS], UC.strangers()
    pre = (np.arange(UC.STRANGERS) % 2).astype(np.uint8)
    ctx.stream_inspect_load(task_id=np.array(ids, np.uint64), started_at=np.full(len(ids), 65, np.int64),
                            env_id=np.zeros(len(ids), np.uint32), requestor_ip=np.array(new, np.uint32), prefetch=pre)
    L = {t: (ip, False, False) for t, ip in whose.items()}
    L.update({t: (ip, False, bool(p)) for t, ip, p in zip(ids, new, pre.tolist())})
    _after_the_strangers(ctx, exp, list(L.values()), UC.STRANGERS)


def test_inspect_restore_with_usage_on_names_requestors_the_table_has_not_met():
    """The same through a full sidecar (snapshot.build_inspect_delta) and ydc_stream_inspect_restore, which
    keeps usage on: every record of L is written, 520 of them with new requestors."""
    ctx, exp, whose = _ramped()
    state = snapshot.apply_inspect_delta(None, ctx.stream_delta_inspect())
    ids = state["task_id"].tolist()
    assert ids == sorted(whose)
    new = UC.strangers()
    state["requestor_ip"] = np.array(new + [whose[t] for t in ids[UC.STRANGERS:]], np.uint32)
    state["prefetch"] = (np.arange(len(ids)) % 3 == 0).astype(np.uint8)
    ctx.stream_inspect_restore(snapshot.build_inspect_delta(state, None, snapshot.INSPECT_FULL))
    same(ctx, exp, new[:40], "behind the restore: usage is still on")
    L = [(int(ip), False, bool(p)) for ip, p in zip(state["requestor_ip"].tolist(), state["prefetch"].tolist())]
    _after_the_strangers(ctx, exp, L, len(ids))  # (a full sidecar files every record of L)
