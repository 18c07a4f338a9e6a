"""The digest index over the book, the load per requestor and the tick's quota table (book_index.h,
requestor_index.h, stream_quota.h, stream_fair.h) walked along chains: keys and requestor ids computed
to share a home slot (tests/hash_index_cases.py, pinned by tests/test_hash_index_model.py), so that a
probe walks a long run, a miss walks a run to its end, the run goes from the last slot to slot 0, the
64 lanes of a wave race for one free slot, and a chain splits or stays when the table doubles. The
keys of the other suites land in their home slot or one or two further.

Every answer is compared with the existing models, integer for integer, through the helpers and rigs
of the suites of the three tables: ask / same_hits (tests/test_stream_book_find_gpu.py), check
(tests/test_stream_requestor_gpu.py), Rig.tick (tests/test_stream_quota_gpu.py, _fair_gpu.py). Every
case first asserts, through the restatement, that its keys are on the path it was made for: the slot
count, the run, the largest displacement. Which key sits in which slot is nobody's business here; the
order of ydc_stream_requestor_get's rows is used once, as evidence that the chains lie where the
restatement says, and for nothing else."""
import ctypes as C

import numpy as np
import pytest

from tests import hash_index_cases as H
from tests import stream_book_find_model as FM
from tests import stream_lease_cases as cases
from tests import stream_lease_model as L
from tests import stream_requestor_model as QM
from tests import test_stream_book_find_gpu as BF
from tests import test_stream_fair_gpu as TF
from tests import test_stream_quota_gpu as TQ
from tests import test_stream_requestor_gpu as RQ
from tests.test_stream_book_gpu import Booked
from tests.test_stream_reserve_gpu import new_ctx
from yadcc_amd import binding

pytestmark = pytest.mark.gpu
BITS = H.FLOOR_BITS
SIZE = 1 << BITS
ALL = H.ALL
WAITING, UNKNOWN = RQ.WAITING, RQ.UNKNOWN


# ---- the digest index over the book ---------------------------------------------------------------

class Book:
    """tests/test_stream_book_find_gpu.py's test_exact_sizes_with_hand_made_keys as a vehicle: tick 0
    grants one task, then its servant lists that id m times with the key column staged, so B is exactly
    that column."""

    def __init__(self):
        ls = cases.small_stream()
        ctx = new_ctx(ls.es.sv)
        ctx.stream_begin_leased(ls.es.hb + 8, 16, cases.MAX_TASKS, 64, 64, 64, ls.es.n, 2049)
        self.b, self.ls, self.ctx = Booked("leased", ls, ctx, 2 * 2049), ls, ctx
        r = self.b.tick(cases.scripted(ls, ls.next_tick(), n=1, lease=[10 ** 6]))
        assert int((r["out"] < L.IDX_ENV_NOT_FOUND).sum()) == 1
        (self.s, (self.tid,)), = cases.held(ls.table).items()

    def put(self, col):
        """B becomes `col`. -> the model's columns."""
        col = np.asarray(col, np.uint64)
        m = len(col)
        ev = cases.scripted(self.ls, self.ls.next_tick(), reports=[(self.s, [self.tid] * m)])
        stid = np.arange(m, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)
        self.ctx.stream_book_stage(stid, col)
        self.b.book.stage(stid, col)
        r = self.b.tick(ev, stage=False)
        assert r["unknown_reported"] == 0 and len(self.b.book) == m
        cols = self.b.book.columns()
        assert np.array_equal(cols[3], col)
        return cols

    def ask(self, what, absent, distinct, entries):
        """Every key of B forwards, then everything backwards, the absent keys, 0 and all ones, distinct
        (BF.ask); the absent keys are misses in the model, so they must be on the device."""
        cols = self.b.book.columns()
        miss = FM.find(cols, np.asarray(absent, np.uint64))
        assert (miss["pos"] == FM.NOT_FOUND).all() and not miss["count"].any(), what
        fold = BF.ask(self.ctx, self.b.book, what, rebuilt=True, extra=np.asarray(absent, np.uint64))
        assert len(fold[0]) == distinct and int(fold[4].sum()) == entries, what
        return fold

    def close(self):
        self.b.close()


@pytest.mark.parametrize("h", H.HOMES)
def test_book_chains_of_one_home(h):
    """B holds a chain of 1 .. 257 keys of one home once, in key order and shuffled. Asked: every member
    forwards and backwards; 16 absent keys of the same home, which walk the whole run (across the wrap at
    1021 and 1023) and miss; absent keys whose home is inside the run (h + 1, h + n - 1) and at its first
    free slot (h + n); 0 and all ones. Then distinct."""
    bk = Book()
    rng = np.random.default_rng(h)
    for n in H.LENGTHS:
        keys = H.key_colliders(BITS, h, n)
        assert H.slots_book(n) == SIZE
        run = H.one_chain(keys, BITS, h)
        assert (SIZE - 1 in run and 0 in run) == (h + n > SIZE)
        absent = H.absent_around(BITS, h, n, keys)
        assert sum(H.home(k, BITS) == h for k in absent) >= 16
        for order, col in (("key order", sorted(keys)), ("shuffled", [keys[i] for i in rng.permutation(n)])):
            bk.put(col)
            bk.ask("home %d, %d keys, %s" % (h, n, order), absent, n, n)
    bk.close()


@pytest.mark.parametrize("h", H.HOMES)
def test_book_duplicates_on_a_chain(h):
    """Each member of a chain is in B once, twice or three times, at scattered positions: a wave holds
    equal keys and distinct keys of one home at once. last1 is the largest position, count is exact."""
    bk = Book()
    rng = np.random.default_rng(h + 1)
    for n in (2, 63, 65, 170):
        keys = np.array(H.key_colliders(BITS, h, n), np.uint64)
        H.one_chain(keys.tolist(), BITS, h)
        reps = 1 + np.arange(n) % 3
        col = np.repeat(keys, reps)[rng.permutation(int(reps.sum()))]
        m = len(col)
        assert H.slots_book(m) == SIZE and m > n
        bk.put(col)
        what = "home %d, %d keys in %d entries" % (h, n, m)
        bk.ask(what, H.absent_around(BITS, h, n, keys.tolist()), n, m)
        got, built = bk.ctx.stream_book_find(keys)
        assert not built
        last = np.array([np.nonzero(col == k)[0].max() for k in keys], np.uint32)
        assert np.array_equal(got["count"], reps.astype(np.uint32)) and np.array_equal(got["pos"], last), what
    bk.close()


@pytest.mark.parametrize("h", H.HOMES)
def test_book_all_ones_amid_a_chain(h):
    """All ones, the index's free-slot mark, three times among 65 keys of one home: it goes to the side
    record and the chain around it is whole."""
    bk = Book()
    keys = H.key_colliders(BITS, h, 65)
    H.one_chain(keys, BITS, h)
    col = list(keys)
    for at in (3, 30, 67):
        col.insert(at, ALL)
    assert len(col) == 68 and col[67] == ALL
    bk.put(col)
    bk.ask("home %d, all ones amid the chain" % h, H.absent_around(BITS, h, 65, keys), 66, 68)
    got, _ = bk.ctx.stream_book_find(np.array([ALL] + keys, np.uint64))
    assert (got["pos"][0], got["count"][0]) == (67, 3) and (got["count"][1:] == 1).all()
    assert np.array_equal(got["pos"][1:], [col.index(k) for k in keys])
    bk.close()


@pytest.mark.parametrize("h", [100, 1010])
def test_book_two_chains_whose_runs_touch(h):
    """40 keys at h and 40 at h + 20: one run of 80 (across the wrap from 1010). A key's walk goes on
    through the other chain's members; absent keys of both homes walk to the end of the run."""
    bk = Book()
    h2 = (h + 20) % SIZE
    pool_a, pool_b = H.key_colliders(BITS, h, 56), H.key_colliders(BITS, h2, 56)
    a, b = pool_a[:40], pool_b[:40]
    absent = pool_a[40:] + pool_b[40:] + H.key_colliders(BITS, (h + 80) % SIZE, 1)
    rng = np.random.default_rng(h)
    for order, col in (("first chain first", a + b), ("second chain first", b + a),
                       ("shuffled", [(a + b)[i] for i in rng.permutation(80)])):
        occ, md = H.layout(col, BITS)
        assert occ == H.run_of(h, 80, BITS) and md > 39, "not one run longer than either chain"
        bk.put(col)
        bk.ask("chains at %d and %d, %s" % (h, h2, order), absent, 80, 80)
    bk.close()


@pytest.mark.parametrize("kind", ["split", "stay1"])
@pytest.mark.parametrize("h", H.HOMES)
def test_book_chain_when_the_table_doubles(h, kind):
    """512 keys of one home in 1024 slots: load exactly 1/2, displacements up to 511. One more and the
    table has 2048 slots: keys that differ in bit 10 of the mix are two chains then, at h and h + 1024;
    keys that share it are still one (at h + 1024, across the wrap of the larger table from 1021 and 1023)."""
    bk = Book()
    pool = H.key_colliders(BITS, h, 513 + 16, kind=kind)
    keys, absent = pool[:513], pool[513:]
    rng = np.random.default_rng(h)
    assert H.slots_book(512) == SIZE and H.slots_book(513) == 2 * SIZE
    H.one_chain(keys[:512], BITS, h)
    bk.put([keys[i] for i in rng.permutation(512)])
    bk.ask("home %d, 512 keys" % h, absent + H.absent_around(BITS, h, 512, keys[:512], same=0), 512, 512)
    homes = {h: 257, h + SIZE: 256} if kind == "split" else {h + SIZE: 513}
    occ, md = H.layout(keys, BITS + 1)
    assert occ == frozenset().union(*[H.run_of(hh, n, BITS + 1) for hh, n in homes.items()])
    assert md == max(homes.values()) - 1 and len(occ) == 513
    assert {H.home(k, BITS + 1) for k in absent} == set(homes)
    bk.put([keys[i] for i in rng.permutation(513)])
    bk.ask("home %d, 513 keys, %s" % (h, kind), absent, 513, 513)
    bk.close()


# ---- the load per requestor -----------------------------------------------------------------------

def rpc_ctx(sv, inspect=False):
    ctx = RQ.uploaded(sv)
    ctx.stream_begin_rpc(8, 16, 600, 1 << 13, 1100, 1 << 14, 8, 8, 8, 8)
    if inspect:
        ctx.stream_inspect_begin()
    return ctx


def wait_all(ctx, now, ips, first_tag, rng, before):
    """Every id of `ips` sends one RPC that has to wait. -> |W|."""
    r = RQ.rpc_tick(ctx, now, RQ.rpc_requests(ips, first_tag, rng))
    assert (r["status"] == WAITING).all() and r["n_waiting"] == before + len(ips)
    return r["n_waiting"]


def waiting_model(ctx, n):
    model, un = QM.fold(None, ctx.stream_waiting())
    assert len(model) == n and un == UNKNOWN and H.slots_requestor(int(model["waiting"].sum())) == SIZE
    return model, un


def raw_rows(ctx):
    """ydc_stream_requestor_get as the library answers it: the rows in slot order."""
    lib, n, un = binding.lib(), C.c_uint32(0), C.c_uint32(0)
    assert lib.ydc_stream_requestor_get(ctx._h, None, 0, C.byref(n), C.byref(un)) == RQ.CAPACITY and n.value
    room = np.zeros(n.value, QM.DTYPE)
    assert lib.ydc_stream_requestor_get(ctx._h, room.ctypes.data, n.value, C.byref(n), C.byref(un)) == 0
    assert n.value == len(room)
    return room["requestor_ip"].tolist()


@pytest.mark.parametrize("combine", [None, "0"])
@pytest.mark.parametrize("h", H.HOMES)
def test_requestor_chain_in_the_waiting_queue(h, combine, monkeypatch):
    """W of a saturated rpc stream, where position i is lane i % 64: 64 distinct requestors of one home
    in one wave (four combine rounds, then 60 lanes race for one run), then 257 of that home over five
    waves and two workgroups. With equal requestors combined inside the wave and with an atomic per
    entry. find: the members, absent ids of the same home, absent ids whose home is inside the run, the
    ids nobody has; get: the model's fold."""
    if combine is not None:
        monkeypatch.setenv("YDC_REQUESTOR_COMBINE", combine)
    chain = H.ip_colliders(BITS, h, 257)
    rng = np.random.default_rng(h)
    ctx = rpc_ctx(RQ.saturated_registry())
    n_w = 0
    for n, now in ((64, 10), (257, 11)):
        H.one_chain(chain[:n], BITS, h)
        new = chain[n_w:n]
        n_w = wait_all(ctx, now, [new[i] for i in rng.permutation(len(new))], 1 + n_w, rng, n_w)
        model, un = waiting_model(ctx, n)
        absent = H.absent_around(BITS, h, n, chain[:n], ids=True)
        g = RQ.check(ctx, model, un, absent, "home %d, %d requestors in W" % (h, n))
        assert set(g["requestor_ip"].tolist()) == set(chain[:n]) and (g["waiting"] == 1).all()
    ctx.stream_end()
    ctx.close()


def test_requestor_rows_come_in_slot_order_from_the_runs_the_restatement_predicts():
    """The evidence that the chains lie where the restatement puts them: with two chains that do not touch
    and nothing else in the table, the first n1 rows of the raw call are the lower chain's ids as a set;
    a chain at 1021 has its wrapped members in front of everybody and its first three behind."""
    rng = np.random.default_rng(4)
    for (h1, n1), (h2, n2) in (((300, 5), (700, 7)), ((500, 5), (1021, 64)), ((100, 64), (1023, 65))):
        a, b = H.ip_colliders(BITS, h1, n1), H.ip_colliders(BITS, h2, n2)
        occ, _ = H.layout(a + b, BITS)
        assert occ == H.run_of(h1, n1, BITS) | H.run_of(h2, n2, BITS) and len(occ) == n1 + n2
        ctx = rpc_ctx(RQ.saturated_registry())
        both = a + b
        wait_all(ctx, 10, [both[i] for i in rng.permutation(n1 + n2)], 1, rng, 0)
        rows = raw_rows(ctx)
        wrapped = max(0, h2 + n2 - SIZE)  # members of the upper chain in slots 0 ..
        assert wrapped == {700: 0, 1021: 61, 1023: 64}[h2]
        assert set(rows[wrapped:wrapped + n1]) == set(a), "the lower chain is not where the restatement puts it"
        assert set(rows[:wrapped]) | set(rows[wrapped + n1:]) == set(b) and len(rows) == n1 + n2
        ctx.stream_end()
        ctx.close()


@pytest.mark.parametrize("h", [100, 1021])
def test_requestor_chain_in_the_lease_table(h):
    """257 requestors of one home with 1 .. 3 leases each, granted to an rpc stream: prefetch leases among
    them, and every other requestor's have run out by the second tick (zombies)."""
    chain = np.array(H.ip_colliders(BITS, h, 257), np.uint32)
    H.one_chain(chain.tolist(), BITS, h)
    rng = np.random.default_rng(h)
    ips = chain[rng.permutation(257)]
    i = np.arange(257)
    req = {"env_id": np.zeros(257, np.uint32), "min_version": np.zeros(257, np.uint32), "requestor_ip": ips,
           "n_immediate": np.ones(257, np.uint32), "n_prefetch": np.array([0, 0, 1, 2], np.uint32)[i % 4],
           "lease_for": np.where(i % 2 == 0, 5, 1000).astype(np.int64), "deadline": np.full(257, 1 << 40, np.int64),
           "tag": np.arange(1, 258, dtype=np.uint64)}
    rows = int(req["n_immediate"].sum() + req["n_prefetch"].sum())
    assert 257 < rows <= 512 and H.slots_requestor(rows) == SIZE
    ctx = rpc_ctx(RQ.roomy_registry(), inspect=True)
    r = RQ.rpc_tick(ctx, 10, req)
    assert r["n_waiting"] == 0 and not (r["status"] == WAITING).any() and int(r["n_granted"].sum()) == rows
    r = RQ.rpc_tick(ctx, 20, RQ.rpc_requests([], 300, rng))
    tasks = ctx.stream_inspect_tasks()
    assert len(tasks["requestor_ip"]) == rows, "a lease was swept: the table no longer holds the chain's"
    model, un = QM.fold(tasks, ctx.stream_waiting())
    assert un == 0 and len(model) == 257
    g = RQ.check(ctx, model, un, H.absent_around(BITS, h, 257, chain.tolist(), ids=True), "home %d, 257 requestors in L" % h)
    assert int(g["leases"].sum()) == rows and set(g["leases"].tolist()) == {1, 2, 3}
    assert 0 < int(g["zombies"].sum()) < rows and int(g["prefetch_leases"].sum()) == int(req["n_prefetch"].sum())
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("h", [100, 1021])
def test_requestor_chain_with_leases_and_waiting_calls(h):
    """The same chain's requestors hold leases AND wait: a slot claimed by k_requestor_leases is found by
    k_requestor_waiting, and the other way round for those that only wait."""
    chain = H.ip_colliders(BITS, h, 200)
    H.one_chain(chain, BITS, h)
    rng = np.random.default_rng(h)
    ctx = rpc_ctx(RQ.roomy_registry(16), inspect=True)  # 128 slots
    ips = np.array(chain[:128], np.uint32)[rng.permutation(128)]
    req = RQ.rpc_requests(ips, 1, rng)
    req["env_id"][:], req["n_immediate"][:], req["n_prefetch"][:] = 0, 1, 0
    r = RQ.rpc_tick(ctx, 10, req)
    assert int(r["n_granted"].sum()) == 128 and r["n_waiting"] == 0
    wait_all(ctx, 11, [chain[i] for i in rng.permutation(200)], 1000, rng, 0)
    assert H.slots_requestor(128 + 200) == SIZE
    model, un = QM.fold(ctx.stream_inspect_tasks(), ctx.stream_waiting())
    assert un == 0 and len(model) == 200
    g = RQ.check(ctx, model, un, H.absent_around(BITS, h, 200, chain, ids=True), "home %d, L and W" % h)
    assert int(((g["leases"] == 1) & (g["waiting"] == 1)).sum()) == 128 and int((g["leases"] == 0).sum()) == 72
    ctx.stream_end()
    ctx.close()


def test_requestor_ids_0_and_all_ones_as_members_of_chains():
    """0 (whose home is slot 0) and 0xFFFFFFFF (YDC_INSPECT_NO_ID, an ordinary key here) each amid 63
    other ids of their home."""
    hf = H.home(0xFFFFFFFF, BITS)
    zero, ones = [0] + H.ip_colliders(BITS, 0, 63), [0xFFFFFFFF] + H.ip_colliders(BITS, hf, 63)
    H.one_chain(zero, BITS, 0)
    H.one_chain(ones, BITS, hf)
    assert H.layout(zero + ones, BITS)[0] == H.run_of(0, 64, BITS) | H.run_of(hf, 64, BITS) and 64 < hf < SIZE - 64
    rng = np.random.default_rng(6)
    ctx = rpc_ctx(RQ.saturated_registry())
    both = zero + ones
    wait_all(ctx, 10, [both[i] for i in rng.permutation(128)], 1, rng, 0)
    model, un = waiting_model(ctx, 128)
    absent = H.absent_around(BITS, 0, 64, zero, ids=True) + H.absent_around(BITS, hf, 64, ones, ids=True)
    g = RQ.check(ctx, model, un, absent, "0 and 0xFFFFFFFF on chains")  # (check asks for 0, 0xFFFFFFFE, 0xFFFFFFFF too)
    assert {0, 0xFFFFFFFF} <= set(g["requestor_ip"].tolist()) and (g["waiting"] == 1).all()
    rows = raw_rows(ctx)
    assert set(rows[:64]) == set(zero) and set(rows[64:]) == set(ones)
    ctx.stream_end()
    ctx.close()


@pytest.mark.parametrize("kind", ["split", "stay1"])
@pytest.mark.parametrize("h", [100, 1021])
def test_requestor_chain_when_the_table_doubles(h, kind):
    """|W| = 512 requestors of one home: 1024 slots at load 1/2. One more: 2048 slots, and the chain
    splits (h and h + 1024) or stays (h + 1024) as bit 10 of the mix says."""
    pool = H.ip_colliders(BITS, h, 513 + 16, kind=kind)
    chain, absent = pool[:513], pool[513:]
    H.one_chain(chain[:512], BITS, h)
    homes = {h: 257, h + SIZE: 256} if kind == "split" else {h + SIZE: 513}
    occ, md = H.layout(chain, BITS + 1)
    assert occ == frozenset().union(*[H.run_of(hh, n, BITS + 1) for hh, n in homes.items()]) and md == max(homes.values()) - 1
    assert H.slots_requestor(512) == SIZE and H.slots_requestor(513) == 2 * SIZE
    rng = np.random.default_rng(h)
    ctx = rpc_ctx(RQ.saturated_registry())
    wait_all(ctx, 10, [chain[i] for i in rng.permutation(512)], 1, rng, 0)
    model, un = waiting_model(ctx, 512)
    RQ.check(ctx, model, un, absent + H.absent_around(BITS, h, 512, chain[:512], same=0, ids=True), "home %d, |W| = 512" % h)
    wait_all(ctx, 11, chain[512:], 2000, rng, 512)
    model, un = QM.fold(None, ctx.stream_waiting())
    assert len(model) == 513 and un == UNKNOWN
    g = RQ.check(ctx, model, un, absent, "home %d, |W| = 513, %s" % (h, kind))
    assert set(g["requestor_ip"].tolist()) == set(chain)
    if kind == "split":  # (slot order, as evidence: the 257 that stay at h lie in front of the 256 that moved,
        rows = raw_rows(ctx)  # but for those of the moved that went on from the last slot to slot 0)
        wrapped = max(0, h + SIZE + 256 - 2 * SIZE)
        assert wrapped == {100: 0, 1021: 253}[h]
        assert {H.home(ip, BITS + 1) for ip in rows[wrapped:wrapped + 257]} == {h}
        assert {H.home(ip, BITS + 1) for ip in rows[:wrapped] + rows[wrapped + 257:]} == {h + SIZE} and len(rows) == 513
    ctx.stream_end()
    ctx.close()


# ---- the tick's quota table -----------------------------------------------------------------------

PER_TICK = 512  # max_tasks of every rig here: quota_slots(512) == 1024
CAPS = (4, 1, 0, 6, 0, 3, 2, 1)  # overrides of the chain's first members, who hold 0, 1, 2, 3, 0, 1, 2, 3: on both sides


def quota_sets(h, n):
    """The chain that asks in ticks 2 and 4; requestors that hold leases and never ask: 16 of the same
    home, and some whose home is inside the run; tick 3's askers: other ids of the same home and three of
    the chain."""
    pool = H.ip_colliders(BITS, h, n + 16 + max(1, n // 2))
    chain, same, fresh = pool[:n], pool[n:n + 16], pool[n + 16:]
    inside = []
    for hh in sorted({(h + 1) % SIZE, (h + n // 2) % SIZE, (h + n - 1) % SIZE} - {h}):
        inside += H.ip_colliders(BITS, hh, 2)
    H.one_chain(chain, BITS, h)
    assert all(H.home(ip, BITS) == h for ip in same + fresh) and all(H.home(ip, BITS) in H.run_of(h, n, BITS) for ip in inside)
    third = fresh + [chain[i] for i in sorted({1 % n, 2 % n, n - 1})]
    H.one_chain(third, BITS, h)
    return chain, same + inside, third


def asking(mode, ids, total, rng):
    """`total` requests (at least one pass) of the ids, pass after pass in a new order each: every id asks
    several times, in several waves and, beyond 256 requests, in both tiles of the clip pass."""
    order = []
    while len(order) < max(total, len(ids)):
        order += [ids[i] for i in rng.permutation(len(ids))]
    order = order[:max(total, len(ids))]
    if mode == "wl":
        return [(ip, 1, 0) for ip in order]
    return [(ip, 1 + j % 2, j % 3) for j, ip in enumerate(order)]


def quota_script(rig, mode, h, n):
    """Four ticks through Rig.tick. 1: the lease table fills (the chain's member i holds i % 4, the others
    one each). 2: the chain asks under a default cap of 2 and overrides on both sides of what their members
    hold. 3: a shorter set of the same home asks, disjoint but for three members. 4: tick 2's set again."""
    assert H.slots_quota(PER_TICK) == SIZE
    chain, others, third = quota_sets(h, n)
    rng = np.random.default_rng(1000 * h + n)
    rig.set(TQ.UNL)
    if mode == "wl":
        fill = [(ip, 1, 0) for i, ip in enumerate(chain) for _ in range(i % 4)]
    else:
        fill = [(ip, 1, i % 4 - 1) for i, ip in enumerate(chain) if i % 4]
    fill = [fill[i] for i in rng.permutation(len(fill))] + [(ip, 1, 0) for ip in others]
    assert len(fill) <= PER_TICK
    rig.tick(rig.event(fill), snapshot=False)
    held = sum(i % 4 for i in range(n)) + len(others)
    assert len(rig.held()) == held and rig.q.result[2] == 0
    total = {2: 300, 64: 320, 65: 325, 257: 512}[n]
    second = asking(mode, chain, total, rng)
    assert 256 < len(second) <= PER_TICK
    rig.set(2, {chain[i]: CAPS[i] for i in range(min(n, len(CAPS)))})
    seen = []
    for t, reqs in ((2, second), (3, asking(mode, third, 2 * len(third), rng)), (4, second)):
        free = rig.held()[::2] if t == 4 else []  # (half of everything goes back: there is room again, member by member)
        rig.tick(rig.event(reqs, free=free), snapshot=t == 4)
        m_imm, m_pre, clipped, refused = rig.q.result
        admitted = int(m_imm.sum() + m_pre.sum())
        seen.append((clipped, refused, admitted))
        # (what the members hold and ask decides, slot by slot)
        assert clipped > 0 and refused > 0 and admitted > 0 and refused < len(reqs), (t, seen)
        held += admitted - len(free)
        assert len(rig.held()) == held, "tick %d: an admitted row was not granted" % t
    return seen


def quota_rig(mode, cls=TQ.Rig):
    return cls(mode, TQ.tiny_pool(8, 1200), PER_TICK + 64, PER_TICK, max_rows=8192, max_leases=1 << 14)


@pytest.mark.parametrize("n", [2, 64, 65, 257])
@pytest.mark.parametrize("h", H.HOMES)
@pytest.mark.parametrize("mode", TQ.MODES)
def test_quota_table_with_the_askers_of_one_home(mode, h, n):
    """n requestors of one home ask in one tick: k_quota_claim's lanes race for one run; k_quota_loads
    looks up every holder of a lease, and those that do not ask walk the run and miss; the clip pass and
    the label read `held` and `asked` of exactly the request's own slot; k_quota_label leaves the table
    clear for a shorter chain of the same home and for the first one again."""
    rig = quota_rig(mode)
    quota_script(rig, mode, h, n)
    rig.close()


def test_quota_table_with_the_step_enqueued_kernel_by_kernel(monkeypatch):
    TQ._graph(monkeypatch, "0")
    rig = quota_rig("rpc")
    quota_script(rig, "rpc", 1021, 65)
    rig.close()


@pytest.mark.parametrize("h", [100, 1021])
@pytest.mark.parametrize("mode", TQ.MODES)
def test_fair_level_over_257_askers_of_one_home(mode, h):
    """tests/test_stream_fair_gpu.py's test_distinct_askers_in_one_tick with 257 askers of one home and its
    fixed pool; three overrides sit on chain members. k_fair_level walks the slots: the level, n_askers and
    n_override_askers are the model's wherever the chain lies."""
    chain = H.ip_colliders(BITS, h, 257)
    H.one_chain(chain, BITS, h)
    if mode == "wl":
        crowd = [(ip, 1, 0) for i, ip in enumerate(chain) for _ in range(1 + i % 2)]
    else:
        crowd = [(ip, 1 + i % 2, i % 3) for i, ip in enumerate(chain)]
    per_tick = len(crowd)
    assert H.slots_quota(per_tick) == SIZE
    rig = TF.Rig(mode, TQ.tiny_pool(8, 1200), per_tick + 64, per_tick, max_rows=8192, max_leases=1 << 14)
    rig.set(TQ.UNL, {chain[1]: 1, chain[64]: 2, chain[256]: 0})
    levels = []
    for rep in range(2):
        held = rig.held()
        ev = rig.event(crowd, wait=0, free=held[::2])
        rows = len(ev["tags"]) if mode == "wl" else int(ev["n_immediate"].sum() + ev["n_prefetch"].sum())
        rig.fair(TF.FIX, (len(held) - len(held[::2]) + rows) * 2 // 3, 0)
        r = rig.tick(ev, snapshot=False)
        assert (r["fair"]["n_askers"], r["fair"]["n_override_askers"]) == (257, 3)
        levels.append(r["fair"]["level"])
    assert set(levels) - {TQ.UNL}, levels
    rig.close()
