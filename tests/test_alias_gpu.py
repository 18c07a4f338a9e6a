"""Host aliases (ydc_set_host_aliases) on the device, pinned to the reference at batch size.

Every case of tests/alias_cases.py — servants by location STRING, requests by requestor address
STRING, interned by tests/alias_reference.py — goes through the C ABI: upload_servants, then
set_host_aliases, then the call under test. servant_idx, the utilisation doubles (bit for bit) and
running_tasks must EQUAL the reference's (tests/alias_reference.py, or the verbatim reference class
beyond its size limit; tests/test_alias_model.py holds the two together on the CPU, and shows
that in every case the aliases decide placements).

Which code ran is asserted from stats() / kernel_profile() / debug_pipeline() in every test. One
thing follows from the product and not from these tests: a context with a non-empty alias list
never takes the one-workgroup tick kernel (tick_takes, ydc_api.hip), so a batch of 1, 63 or 64
requests and every ydc_dispatch_tick turn is placed by the batch pipeline; the tests assert that
routing (small_batch == 0, no resident and no launched tick call) and that the same turns without
the list do take the tick kernel.

Wall time on one MI355X, measured once: 3.1 s for the file's 62 tests; the longest are the 66-case
fuzz (0.55 s) and the first test of the file (0.27 s, with the first context of the process).
"""
import copy
import time

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import alias_cases as K
from tests import alias_reference as A
from tests import class_edge_cases as CE
from tests.test_class_edges_gpu import PROFILE_OF, ran
from tests.test_sharded_gpu import sharded_run
from yadcc_amd import binding, pack

pytestmark = pytest.mark.gpu

DA = binding.DeviceArray
COLS = ("env_id", "min_version", "requestor_ip")
ENF = A.IDX_ENV_NOT_FOUND
BIG = tuple([k for k in K.RANDOM_SPECS if k[1:] == shape][0] for shape in ((300, 5000), (40, 5000)))


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.perf_counter()
    yield
    print("[time] %s %.2f s" % (request.node.name, time.perf_counter() - t0))


def prefix_want(case, n):
    """A sequential batch's prefix is the prefix batch: the reference's answers for the first n
    requests and running_tasks after them."""
    idx, util, _ = K.want(case)
    run = np.asarray(case.sv["running_tasks"], np.int64).copy()
    np.add.at(run, idx[:n][idx[:n] < ENF].astype(np.int64), 1)
    return idx[:n], util[:n], run.astype(np.uint32)


def context(monkeypatch, case, aliases=True, n_upload=None, **switches):
    for k, v in switches.items():
        monkeypatch.setenv("YDC_" + k, str(v))
    c = binding.Context(device=0)
    c.set_profiling(True)
    load(c, case, aliases, n_upload)
    return c


def load(c, case, aliases=True, n_upload=None):
    cols = pack.to_abi_columns(case.sv)
    if n_upload is not None:
        cols = {k: v[:n_upload] for k, v in cols.items()}
    c.upload_servants(cols)
    if aliases:
        c.set_host_aliases(*case.aliases)


def expected_kernel(case, n, **switches):
    """The matching kernel of the batch pipeline for this registry (tests/class_edge_cases.py:
    plan_of), with a path switched off where the test does that."""
    path = CE.plan_of(case.sv, n)["kernel"]
    if path == CE.MATCH:
        return "k_match_pass"
    if switches.get("WIDE") == 0 or path == CE.GENERIC:
        return "k_sim_generic"
    if switches.get("GROUP_WALK") == 0 or path == CE.WIDE:
        return "k_sim_wide"
    return PROFILE_OF[path]


def check(c, case, lo, hi, want, commit=False, kernel=None, where=None):
    """Requests lo .. hi in one ydc_dispatch; want = (idx, util, running after)."""
    tk = case.slice(lo, hi)[1]
    got, gutil, grun = c.dispatch(tk, commit=commit)
    st, prof = c.stats(), c.kernel_profile()
    ctx = (case, lo, hi, where, st)
    bad = np.nonzero(got != want[0])[0]
    assert bad.size == 0, (ctx, bad[:5], got[bad[:5]], want[0][bad[:5]], [case.requestors[lo + t] for t in bad[:5]])
    assert np.array_equal(gutil, want[1]), ctx
    assert np.array_equal(grun, want[2]), ctx
    assert st["granted"] == int((want[0] < ENF).sum()), ctx
    assert st["timeouts"] == int((want[0] == A.IDX_TIMEOUT).sum()), ctx
    assert st["env_not_found"] == int((want[0] == ENF).sum()), ctx
    assert st["small_batch"] == 0, ctx  # (never the tick kernel while aliases are set)
    if hi > lo and st["n_slots"]:
        assert ran(prof) == {kernel or expected_kernel(case, hi - lo)}, (ctx, sorted(prof))
    return st


# ---------------------------------------------------------------------------------------------
# ydc_dispatch, one batch
# ---------------------------------------------------------------------------------------------
MADE = [f.__name__ for f in K.MADE]


@pytest.mark.parametrize("name", MADE)
def test_one_batch_of_every_made_case(name, monkeypatch):
    case = K.get(name)
    c = context(monkeypatch, case)
    try:
        st = check(c, case, 0, case.n_requests, K.want(case))
        assert np.array_equal(c.get_running(), case.sv["running_tasks"])  # (not committed)
        check(c, case, 0, case.n_requests, K.want(case), commit=True)
        assert np.array_equal(c.get_running(), K.want(case)[2])
        if name == "many_classes":
            assert st["n_classes"] > 256, st
        if name == "huge":
            assert st["key_bits"] == 64, st  # the fp64 key
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("key", BIG, ids=["S300", "S40"])
def test_one_batch_at_the_sizes_where_the_route_changes(key, n, monkeypatch):
    """1, 63, 64: what a context without aliases gives the one-launch tick kernel; 65, 257, 5000:
    the pipeline of several kernels. With aliases all of them are the pipeline's, without (the same
    registry, the list never set) the first three are the tick kernel's."""
    if n == 1:  # (a random case of ONE request, which the alias decides, on as many servants)
        key = [k for k in K.RANDOM_SPECS if k[1:] == (key[1], 1)][0]
    case = K.get(key)
    c = context(monkeypatch, case)
    try:
        st = check(c, case, 0, n, prefix_want(case, n))
        assert st["n_tasks"] == n
        load(c, case, aliases=False)
        got = c.dispatch(case.slice(0, n)[1])[0]
        assert c.stats()["small_batch"] == int(n <= 64), c.stats()
        assert np.array_equal(got, O.dispatch(case.sv, case.slice(0, n)[1], "scan")[0])
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# Forced paths
# ---------------------------------------------------------------------------------------------
SWITCHES = [dict(CHUNK_SIZE=64), dict(CHUNK_SIZE=128), dict(RING_TOTAL=256), dict(BINSORT=0), dict(FUSE_PASSES=0)]
MANY = [dict(WIDE=0), dict(GROUP_WALK=0), dict(WALK_PACKED=0)]
FORCED = ([(k, s) for k in ("bracket", "everybody", "many_classes", BIG[0]) for s in SWITCHES] +
          [("many_classes", s) for s in MANY])


@pytest.mark.parametrize("key,switches", FORCED, ids=["%s-%s" % (k if isinstance(k, str) else "S300N5000",
                                                                 "".join("%s=%s" % kv for kv in s.items()))
                                                      for k, s in FORCED])
def test_forced_paths(key, switches, monkeypatch):
    case = K.get(key)
    c = context(monkeypatch, case, **switches)
    try:
        check(c, case, 0, case.n_requests, K.want(case), commit=True,
              kernel=expected_kernel(case, case.n_requests, **switches), where=switches)
        assert np.array_equal(c.get_running(), K.want(case)[2])
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# Two committed halves
# ---------------------------------------------------------------------------------------------
def cut_inside_a_run(case, who="["):
    """A request index in the middle third with requests from `who` on both sides of it."""
    r, n = case.requestors, case.n_requests
    for t in list(range(n // 3, n)) + list(range(1, n // 3)):
        if r[t - 1] == who and r[t] == who:
            return t
    raise AssertionError("no run of requests from %r in %r" % (who, case))


@pytest.mark.parametrize("name", ["everybody", "bracket", "dedicated", "many_classes"])
def test_two_committed_halves_cut_inside_a_run_from_the_alias(name, monkeypatch):
    case = K.get(name)
    cut = cut_inside_a_run(case)
    whole = K.want(case)
    mid = prefix_want(case, cut)
    c = context(monkeypatch, case)
    try:
        check(c, case, 0, cut, mid, commit=True)
        assert np.array_equal(c.get_running(), mid[2])
        check(c, case, cut, case.n_requests, (whole[0][cut:], whole[1][cut:], whole[2]), commit=True)
        assert np.array_equal(c.get_running(), whole[2])
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# ydc_dispatch_tick
# ---------------------------------------------------------------------------------------------
class Registry:
    """The reference's side of a sequence of turns: locations, raw columns, running_tasks."""

    def __init__(self, case):
        self.case = case
        self.locations = list(case.locations)
        self.sv = {k: np.array(v, copy=True) for k, v in case.sv.items()}
        self.running = np.asarray(case.sv["running_tasks"], np.int64).copy()
        self.held = []

    def rows(self, idx):
        idx = np.asarray(idx, np.int64)
        rows = np.zeros(len(idx), binding.ROW_DTYPE)
        for k, col in (("version", "version"), ("num_processors", "num_processors"), ("current_load", "current_load"),
                       ("max_tasks", "max_tasks"), ("ip_id", "ip"), ("env_mask", "env_mask")):
            rows[k] = self.sv[col][idx]
        rows["flags"] = pack.servant_flags(self.sv)[idx]
        return rows

    def release(self, rng, n):
        rel = [self.held.pop(int(rng.integers(len(self.held)))) for _ in range(min(n, len(self.held)))]
        np.subtract.at(self.running, np.asarray(rel, np.int64), 1)
        return np.asarray(rel, np.uint32)

    def place(self, requestors, tk, same_host=A.is_network_address_equal):
        idx, util, run = A.dispatch(self.locations, self.sv, requestors, tk, running=self.running, same_host=same_host)
        self.running = run.astype(np.int64)
        self.held.extend(int(s) for s in idx if s < ENF)
        return idx, util


def rpc(case, requestor, env, n, minv=0):
    rid = case.names[requestor]
    return [requestor] * n, {"env_id": np.full(n, env, np.uint32), "min_version": np.full(n, minv, np.uint32),
                             "requestor_ip": np.full(n, rid, np.uint32)}


def test_tick_turns_of_identical_requests_from_an_aliased_host(monkeypatch):
    """Turns of 1 .. 16 identical requests from "[" and "[:" (what one RPC sends: the tick kernel's
    merge, where it runs), with releases and heartbeats that change loads only; then a servant on a new
    host joins in a heartbeat, and the aliases are set again. With the alias list set every turn is the
    batch pipeline's; the same turn without the list is taken by the tick kernel."""
    monkeypatch.setenv("YDC_RESIDENT_IDLE_MS", "20000")
    case = K.get("bracket")
    reg = Registry(case)
    rng = np.random.default_rng(7)
    c = context(monkeypatch, case)
    try:
        for turn in range(24):
            n = 1 + turn % 16
            who = ("[", "[:", "[::3]")[turn % 3]
            req, tk = rpc(case, who, turn % 2, n, minv=20 * (turn % 4 == 0))
            rel = reg.release(rng, int(rng.integers(0, 6)))
            upd = np.unique(rng.integers(0, case.n_servants, 3)).astype(np.uint32)
            reg.sv["current_load"][upd] = rng.integers(0, 8, len(upd))
            want, wutil = reg.place(req, tk)
            got, gutil = c.dispatch_tick(tk, upd, reg.rows(upd), rel, commit=True, want_util=True)
            st = c.stats()
            assert np.array_equal(got, want) and np.array_equal(gutil, wutil), (turn, who, got, want, st)
            assert (st["small_batch"], st["tick_resident_calls"], st["tick_launched_calls"]) == (0, 0, 0), (turn, st)
            assert ran(c.kernel_profile()) == {"k_match_pass"}, (turn, c.kernel_profile())
        assert np.array_equal(c.get_running(), reg.running.astype(np.uint32))
        # a structural heartbeat: a servant on a new host is appended (index == count)
        new = case.n_servants
        reg.locations.append("[::99]:8335")
        for k in reg.sv:
            reg.sv[k] = np.append(reg.sv[k], reg.sv[k][0])
        new_id = 0x51515151
        assert new_id not in case.names.values()
        reg.sv["ip"][new] = new_id
        reg.running = np.append(reg.running, 0)
        req, tk = rpc(case, "[", 0, 5)
        got, gutil = c.dispatch_tick(tk, [new], reg.rows([new]), [], commit=True, want_util=True)
        # (heartbeats keep the list; the new row is in nobody's yet: "[" does not avoid it)
        locs = reg.locations
        reg.locations = locs[:new] + ["elsewhere:1"]
        want, wutil = reg.place(req, tk)
        reg.locations = locs
        assert np.array_equal(got, want) and np.array_equal(gutil, wutil), (got, want, c.stats())
        c.set_host_aliases(np.append(case.aliases[0], [case.names["[:"], case.names["["]]).astype(np.uint32),
                           np.append(case.aliases[1], [new, new]).astype(np.uint32))
        for n in (16, 3):
            req, tk = rpc(case, "[", 0, n)
            want, wutil = reg.place(req, tk)
            got, gutil = c.dispatch_tick(tk, commit=True, want_util=True)
            assert np.array_equal(got, want) and np.array_equal(gutil, wutil), (n, got, want, c.stats())
            assert c.stats()["small_batch"] == 0
        assert np.array_equal(c.get_running(), reg.running.astype(np.uint32))
        # the same registry with the list cleared: the tick kernel takes the turn, and stays
        c.set_host_aliases(np.empty(0, np.uint32), np.empty(0, np.uint32))
        c.set_profiling(False)  # (a profiled tick is never resident)
        for k in range(2):
            req, tk = rpc(case, "[", 0, 4)
            want, _ = reg.place(req, tk, same_host=A.is_primary_address)
            got, _ = c.dispatch_tick(tk, commit=True)
            st = c.stats()
            assert np.array_equal(got, want), (got, want, st)
            assert st["small_batch"] == 1 and st["tick_launched_calls"] == 1 and st["tick_resident_calls"] == k, st
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# ydc_dispatch_device_async
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["everybody", "bracket"])
def test_two_batches_outstanding(name, monkeypatch):
    """Two different batches of aliased requestors in flight, twice over, none committed: each is what
    the synchronous call gives on the unchanged registry, and a second lane was used."""
    case = K.get(name)
    cut = cut_inside_a_run(case)
    spans = [(0, cut), (cut, case.n_requests)]
    wants = [A.dispatch(case.locations, case.sv, *case.slice(lo, hi)) for lo, hi in spans]
    c = context(monkeypatch, case)
    try:
        for (lo, hi), w in zip(spans, wants):  # the synchronous calls
            check(c, case, lo, hi, w)
        cols = [[DA.from_numpy(case.slice(lo, hi)[1][k]) for k in COLS] for lo, hi in spans]
        outs = [DA.from_numpy(np.full(spans[b & 1][1] - spans[b & 1][0], 0xDEADBEEF, np.uint32)) for b in range(4)]
        utils = [DA.from_numpy(np.full(spans[b & 1][1] - spans[b & 1][0], -7.0, np.float64)) for b in range(4)]
        runs = [DA.from_numpy(np.full(case.n_servants, 0xDEADBEEF, np.uint32)) for _ in range(4)]
        c.set_profiling(False)  # (a profiled batch is placed when it is waited for, never enqueued)
        before = c.debug_pipeline()
        c.dispatch_device_async(*cols[0], outs[0], utils[0], runs[0])
        for b in range(1, 4):
            c.dispatch_device_async(*cols[b & 1], outs[b], utils[b], runs[b])
            c.dispatch_wait()
        c.dispatch_wait()
        for b in range(4):
            w = wants[b & 1]
            assert np.array_equal(outs[b].numpy(), w[0]), b
            assert np.array_equal(utils[b].numpy(), w[1]), b
            assert np.array_equal(runs[b].numpy(), w[2]), b
        after = c.debug_pipeline()
        print("batches, second lane, misses:", before, "->", after)
        assert after[0] - before[0] >= 4 and after[1] - before[1] >= 1, (before, after)
        assert np.array_equal(c.get_running(), case.sv["running_tasks"])
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# ydc_stream_tick
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream_graph", ["1", "0"], ids=["captured", "eager"])
@pytest.mark.parametrize("name", ["bracket", "everybody"])
def test_twenty_ticks_of_the_plain_stream(name, stream_graph, monkeypatch):
    """Heartbeats (loads; twice a servant changes its class), releases and a batch of the case's
    requests per tick; the heartbeats keep the alias list. The reference is applied tick by tick with
    its own releases."""
    monkeypatch.setenv("YDC_STREAM_GRAPH", stream_graph)
    case = K.get(name)
    reg = Registry(case)
    rng = np.random.default_rng(17)
    per_tick = max(8, case.n_requests // 20)
    c = context(monkeypatch, case)
    try:
        c.stream_begin(8, 64, per_tick)
        from_alias = 0
        for t in range(20):
            take = np.sort(rng.choice(case.n_requests, per_tick - t % 3, replace=False))
            req = [case.requestors[i] for i in take]
            tk = {k: v[take] for k, v in case.tk.items()}
            rel = reg.release(rng, int(rng.integers(0, 40)))
            upd = np.unique(rng.integers(0, case.n_servants, 4)).astype(np.uint32)
            reg.sv["current_load"][upd] = rng.integers(0, 6, len(upd))
            if t in (6, 13):  # a structural heartbeat (another class): the registry route, the list stays
                reg.sv["version"][upd[0]] = 39 - reg.sv["version"][upd[0]]
            want, _ = reg.place(req, tk)
            got = c.stream_tick(upd, reg.rows(upd), rel, tk)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (t, bad[:5], got[bad[:5]], want[bad[:5]], [req[i] for i in bad[:5]], c.stats())
            assert np.array_equal(c.get_running(), reg.running.astype(np.uint32)), t
            st = c.stats()
            assert st["granted"] == int((want < ENF).sum()) and st["small_batch"] == 0, (t, st)
            from_alias += sum(r in ("[", "[:") for r in req)
        assert from_alias >= 20
        c.stream_end()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# ydc_update_servants, ydc_remove_servants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bracket", "chain"])
def test_a_servant_appended_by_update_then_named_by_the_list(name, monkeypatch):
    case = K.get(name)
    last = case.n_servants - 1
    assert last in case.aliases[1]
    c = context(monkeypatch, case, aliases=False, n_upload=last)
    try:
        row = {k: int(pack.to_abi_columns(case.sv)[k][last]) for k in
               ("version", "num_processors", "current_load", "max_tasks", "flags", "ip_id", "env_mask")}
        c.update_servants([last], [row])
        if int(case.sv["running_tasks"][last]):
            c.set_running(case.sv["running_tasks"])
        c.set_host_aliases(*case.aliases)
        check(c, case, 0, case.n_requests, K.want(case), commit=True)
        assert np.array_equal(c.get_running(), K.want(case)[2])
    finally:
        c.close()


def test_removal_drops_the_list_until_it_is_set_again(monkeypatch):
    """ydc_remove_servants drops the alias list (include/yadcc_dispatch.h): the placements directly
    after it are the reference's WITHOUT aliases, and after set_host_aliases in the new numbering
    the reference's with them."""
    case = K.get("bracket")
    gone = [0, 2, 17]
    keep = np.array([s for s in range(case.n_servants) if s not in gone])
    locs = [case.locations[s] for s in keep]
    cols = {k: v[keep] for k, v in case.sv.items()}
    plain = O.dispatch(cols, case.tk, "scan")
    aliased = A.dispatch(locs, cols, case.requestors, case.tk)
    assert int((plain[0] != aliased[0]).sum()) >= case.floor
    new_row = {int(s): i for i, s in enumerate(keep)}
    pairs = [(ip, new_row[int(s)]) for ip, s in zip(*case.aliases) if int(s) in new_row]
    small = copy.copy(case)  # (the same ids: nothing is interned again)
    small.name, small.locations, small.sv, small.n_servants = "bracket-removed", locs, cols, len(keep)
    c = context(monkeypatch, case)
    try:
        check(c, case, 0, case.n_requests, K.want(case))
        c.remove_servants(gone)
        got, gutil, grun = c.dispatch(case.tk)
        assert np.array_equal(got, plain[0]) and np.array_equal(gutil, plain[1]) and np.array_equal(grun, plain[2])
        assert c.stats()["n_servants"] == len(keep)
        c.set_host_aliases(np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32))
        check(c, small, 0, small.n_requests, aliased, commit=True)
        assert np.array_equal(c.get_running(), aliased[2])
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# ydc_group_init_local + ydc_dispatch_sharded
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name", ["bracket", "many_classes"])
def test_sharded_ranks_with_the_list_set_on_each(name, G):
    case = K.get(name)
    want = K.want(case)
    ctxs = [binding.Context(device=0) for _ in range(G)]
    try:
        for c in ctxs:
            load(c, case)
        binding.group_init_local(ctxs)
        n = case.n_requests
        cuts = [0] + [n * (r + 1) // G + (7 if r + 1 < G else 0) for r in range(G)]
        res = sharded_run(ctxs, case.sv, case.tk, cuts, commit=True)
        got = np.concatenate([r[0] for r in res])
        bad = np.nonzero(got != want[0])[0]
        assert bad.size == 0, (case, bad[:5], got[bad[:5]], want[0][bad[:5]], [r[3] for r in res])
        assert np.array_equal(np.concatenate([r[1] for r in res]), want[1])
        for r, c in zip(res, ctxs):
            assert np.array_equal(r[2], want[2])
            assert np.array_equal(c.get_running(), want[2])
            assert c.group_size()[0] == G
        # (sharded: a rank counts its slice; more than 256 classes: the replicated form, every rank
        # places the whole batch and answers its slice)
        granted = int((want[0] < ENF).sum())
        assert sum(r[3]["granted"] for r in res) == (granted * G if res[0][3]["n_classes"] > 256 else granted)
        print("per rank:", [(r[3]["n_tasks"], r[3]["shard_sort_batches"], r[3]["n_classes"]) for r in res])
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------
# A bounded fuzz
# ---------------------------------------------------------------------------------------------
def test_fuzz_sixty_random_cases(monkeypatch):
    """The 60 random cases of tests/alias_cases.py (and the six of one servant), in one context per
    (chunk, rings) pair, a third of them as two committed halves; every mismatch is printed with its
    seed."""
    ctxs, bad, paths = {}, [], {}
    try:
        for i, spec in enumerate(K.RANDOM_SPECS + K.ONE_SERVANT_SPECS):
            rng = np.random.default_rng(spec[0])
            chunk = int(rng.choice([0, 0, 64, 128, 512]))
            rings = int(rng.choice([0, 0, 256, 1024]))
            halves = i % 3 == 0 and spec[2] > 1
            if (chunk, rings) not in ctxs:
                for k, v in (("YDC_CHUNK_SIZE", chunk), ("YDC_RING_TOTAL", rings)):
                    if v:
                        monkeypatch.setenv(k, str(v))
                    else:
                        monkeypatch.delenv(k, raising=False)
                ctxs[(chunk, rings)] = binding.Context(device=0)
                ctxs[(chunk, rings)].set_profiling(True)
            c = ctxs[(chunk, rings)]
            case = K.get(spec)
            want = K.want(case)
            load(c, case)
            n = case.n_requests
            if halves:
                cut = int(rng.integers(1, n))
                a, ua, _ = c.dispatch(case.slice(0, cut)[1], commit=True)
                b, ub, grun = c.dispatch(case.slice(cut, n)[1], commit=True)
                got, gutil = np.concatenate([a, b]), np.concatenate([ua, ub])
            else:
                got, gutil, grun = c.dispatch(case.tk)
            st = c.stats()
            for k in ran(c.kernel_profile()):
                paths[k] = paths.get(k, 0) + 1
            ok = (np.array_equal(got, want[0]) and np.array_equal(gutil, want[1]) and np.array_equal(grun, want[2])
                  and (st["small_batch"] == 0 or len(case.aliases[0]) == 0))  # (a location of one ':' has no alias)
            if not ok:
                first = np.nonzero(got != want[0])[0][:3]
                print("MISMATCH seed %d S %d N %d chunk %d rings %d halves %s first %s stats %s" % (
                    spec + (chunk, rings, halves, first.tolist(), st)))
                bad.append(spec)
        print("matching kernels over the run:", paths)
        assert not bad, bad
        assert "k_match_pass" in paths, paths
    finally:
        for c in ctxs.values():
            c.close()
