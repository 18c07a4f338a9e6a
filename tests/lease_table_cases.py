"""Crafted lease tables: ids that share a home slot, chains across the wrap, and the scripted ticks
that walk them. One list of shapes and one set of scripts, played two ways: through the model alone
(tests/test_lease_table_model.py, which also checks the arithmetic below) and on the GPU against the
model (tests/test_lease_table_gpu.py).

The device's table (yadcc_amd/csrc/lease_table.h) is restated here in plain Python integers, with its
own copy of the constant: cap = max(1024, smallest 2^k >= 2 * max_leases) slots, the home slot of an id
is (id * K mod 2^64) >> (64 - k), linear probing from there, no tombstones, every lookup bounded by the
largest displacement any insert has used. K is odd, so it has an inverse modulo 2^64 and the ids of one
home slot h can be written down: K^-1 * ((h << (64 - k)) + r) for any r < 2^(64 - k). The ids a stream
hands out itself are consecutive and almost never collide under K, so only tables restored from a
blob that holds such ids (yadcc_amd/snapshot.build of tests/stream_snapshot_model.state_of) take the
kernels past a displacement of 1, past a hole inside a chain, or from slot cap - 1 to slot 0.

What the GPU tests may rest on, and nothing more: the SET of occupied slots of a table does not depend
on the order of the inserts (a property of linear probing), and n ids of one home occupy n
consecutive slots from it, so the largest displacement is n - 1 in every order. Which id sits in
which slot is the business of whichever thread won which CAS; nothing here assumes it.

Out of scope: ids at or next to 2^64 - 1. That value is the key of an empty slot, the reference's
counter (one increment per grant) cannot reach it in practice, and ydc_stream_restore takes only ids
below next_id; tests/stream_lease_cases.py (the_empty_slot_key_as_an_id) asks for the marker itself.

A script is a function of a driver `d` and a case: d.tick(n=, lease=, renew=, free=, reports=, ips=)
plays one hand-written tick and returns the model's record, on which the script asserts that the
tick met the situation it was written for (so a case that no longer does fails instead of passing
idly); d.reserve, d.fork, d.base, d.delta, d.only and d.remove are the steps between ticks, which the
model's driver (ModelDriver, below) mostly ignores and the GPU's carries out.
"""
import numpy as np

from tests import stream_lease_cases as lcases
from tests import stream_lease_model as M
from tests import stream_snapshot_model as SM
from yadcc_amd import synth

K = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
K_INV = pow(K, -1, 1 << 64)
assert (K * K_INV) & M64 == 1
FLOOR_BITS = 10        # the table never has fewer than 1024 slots
NEXT_ID = 1 << 62      # next_id of every crafted stream: the ids the ticks hand out go on from here
FAR = 1_000_000        # an expiry no test's clock reaches
MAX_LEASES = 512       # 1024 slots
MAX_TASKS = 256        # requests per tick at most
GRANTS = 200           # the burst of scripts 3, 4 and 7
N_SERVANTS, SLOTS = 48, 16


def cap_bits(max_leases):
    bits = FLOOR_BITS
    while (1 << bits) < 2 * max_leases:
        bits += 1
    return bits


def cap(max_leases):
    return 1 << cap_bits(max_leases)


def home(tid, bits):
    return ((tid * K) & M64) >> (64 - bits)


def colliders(bits, h, n, below=1 << 62):
    """n distinct ids with home(id, bits) == h, below `below`, ascending. The low 64 - bits bits r of
    the product walk the whole range in odd steps, so the ids fall into both halves of the slot's
    interval: some share the next bit of the product as well, some do not."""
    assert 0 <= h < (1 << bits)
    low = 64 - bits
    out, r = set(), 1
    while len(out) < n:
        tid = (K_INV * ((h << low) + r)) & M64
        if tid < below:
            out.add(tid)
        r = (r + 0x2545F4914F6CDD1D) & ((1 << low) - 1)
    return sorted(out)


def probe(ids, bits):
    """The inserts of `ids` in the given order: [(id, slot, displacement)]. The slots of single ids
    depend on the order; see layout() for what does not."""
    mask = (1 << bits) - 1
    taken, out = set(), []
    for tid in ids:
        h = home(tid, bits)
        d = 0
        while (h + d) & mask in taken:
            d += 1
        taken.add((h + d) & mask)
        out.append((tid, (h + d) & mask, d))
    return out


def layout(ids, bits):
    """-> (the set of occupied slots, the largest displacement) after inserting `ids` in the order given."""
    p = probe(ids, bits)
    return frozenset(s for _, s, _ in p), max([d for _, _, d in p] + [0])


def histogram(ids, bits):
    """Displacement -> number of inserts, and under "wrap" the inserts whose probe crossed from the last
    slot to slot 0: the replay behind the table in DESIGN 3.3.2."""
    hist = {}
    for tid, slot, d in probe(ids, bits):
        hist[d] = hist.get(d, 0) + 1
        if slot < home(tid, bits):
            hist["wrap"] = hist.get("wrap", 0) + 1
    return hist


def replay_consecutive(bits, ticks, per_tick, keep=()):
    """The densest shape the suite had before: every tick frees the previous tick's grants (but `keep`)
    and grants per_tick consecutive ids. -> histogram of all inserts."""
    mask = (1 << bits) - 1
    tab, where, hist, nxt, prev = set(), {}, {}, 0, []
    for _ in range(ticks):
        for tid in prev:
            if tid not in keep:
                tab.remove(where.pop(tid))
        prev = []
        for _ in range(per_tick):
            h, d = home(nxt, bits), 0
            while (h + d) & mask in tab:
                d += 1
            tab.add((h + d) & mask)
            where[nxt] = (h + d) & mask
            hist[d] = hist.get(d, 0) + 1
            if d and (h + d) & mask < h:
                hist["wrap"] = hist.get("wrap", 0) + 1
            prev.append(nxt)
            nxt += 1
    return hist


class Case:
    """chains: [(home slot, members)] at `bits`; ids: every member, ascending; spare: one more id of the
    first chain's home that is in no table (a non-member that probes the whole chain)."""

    def __init__(self, name, chains, bits=FLOOR_BITS, ids=None, spare=None):
        self.name, self.chains, self.bits = name, chains, bits
        if ids is None:
            ids = []
            for k, (h, n) in enumerate(chains):
                c = colliders(bits, h, n + (k == 0))
                if k == 0:
                    spare, c = c[n // 2], c[:n // 2] + c[n // 2 + 1:]
                ids += c
        self.ids, self.spare, self.n = sorted(ids), spare, len(ids)
        self.check()

    def run_slots(self):
        """The slots the chains occupy: one run when they touch."""
        return layout(self.ids, self.bits)[0]

    def wraps(self):
        occ = self.run_slots()
        return (1 << self.bits) - 1 in occ and 0 in occ

    def check(self):
        """This case is on the path it was made for."""
        size = 1 << self.bits
        assert len(set(self.ids)) == self.n and self.spare not in self.ids
        assert all(0 <= t < NEXT_ID for t in self.ids + [self.spare])
        want = set()
        for h, n in self.chains:
            assert sum(home(t, self.bits) == h for t in self.ids) == n, self.name
            want |= {(h + d) % size for d in range(n)}
        occ, md = layout(self.ids, self.bits)
        assert home(self.spare, self.bits) == self.chains[0][0]
        if len(self.chains) == 1:
            assert occ == want and md == self.n - 1, self.name

    def hits(self, grants, first=NEXT_ID):
        """Of the ids first .. first + grants - 1: those whose home lies inside the occupied run."""
        occ = self.run_slots()
        return [first + j for j in range(grants) if home(first + j, self.bits) in occ]

    def past_bound(self, grants, first=NEXT_ID):
        """... those that any insertion order files at a displacement above the table's bound so far:
        every slot from the id's home to the end of the run is taken."""
        size = 1 << self.bits
        occ, md = layout(self.ids, self.bits)
        out = []
        for tid in self.hits(grants, first):
            d = 0
            while (home(tid, self.bits) + d) % size in occ:
                d += 1
            if d > md:
                out.append(tid)
        return out


SIZE = 1 << FLOOR_BITS
HOMES = (("mid", 100), ("wrap3", SIZE - 3), ("wrap1", SIZE - 1))
LENGTHS = (1, 2, 63, 64, 65, 257)
CHAINS = [Case("%s_%d" % (name, n), [(h, n)]) for name, h in HOMES for n in LENGTHS]
# Two chains whose runs touch: the second home is the slot directly behind the first run. The table's
# bound is 128, the run is 257 slots long: an id whose home lies early in the run is filed past the bound.
TOUCHING = Case("touching", [(SIZE - 40, 128), ((SIZE - 40 + 128) % SIZE, 129)])
TOUCHING_MID = Case("touching_mid", [(300, 128), (428, 129)])
# A chain of 257 whose home shares its top 11 bits: one chain still after a reserve to 2048 slots.
_whole = colliders(11, 2 * (SIZE - 3) + 1, 258)
WHOLE_2048 = Case("whole_2048", [(SIZE - 3, 257)], ids=_whole[:128] + _whole[129:], spare=_whole[128])
# ... and one that shares only its top 10: two homes after the reserve.
SPLIT_2048 = Case("split_2048", [(SIZE - 3, 257)])
SHAPES = CHAINS + [TOUCHING, TOUCHING_MID, WHOLE_2048, SPLIT_2048]
LONG = [c for c in SHAPES if c.n == 257]
BY_NAME = {c.name: c for c in SHAPES}
assert {home(t, 11) for t in WHOLE_2048.ids} == {2 * (SIZE - 3) + 1}
assert {home(t, 11) for t in SPLIT_2048.ids} == {2 * (SIZE - 3), 2 * (SIZE - 3) + 1}


def crafted_stream(entries, max_leases=MAX_LEASES, n_servants=N_SERVANTS, slots=SLOTS, tasks=MAX_TASKS, seed=42):
    """A small idle pool that max_tasks alone bounds, with the leases `entries` = [(id, servant,
    expires_at, zombie)] in the model's table, running_tasks raised for each, next_id = 2^62.
    -> (the model's stream, the stream's ten bounds): what SM.state_of("leased", ...) needs."""
    sv = synth.make_servants(n_servants, n_tasks_hint=n_servants * slots, n_envs=1, seed=seed)
    sv["num_processors"][:], sv["current_load"][:] = 4096, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = slots, 0
    ls = M.LeaseStream(sv, 0, 0, 0, M.LeaseTable(max_leases), n_envs=1)
    ls.es.hb = 4
    for tid, s, exp, zombie in entries:
        assert 0 <= tid < NEXT_ID and tid not in ls.table.L and 0 <= s < n_servants
        ls.table.L[int(tid)] = [int(s), int(exp), bool(zombie)]
        ls.es.running[s] += 1
    assert (ls.es.running <= sv["max_tasks"]).all(), "more leases on a servant than it has slots"
    assert len(ls.table.L) <= max_leases
    ls.table.next_id = NEXT_ID
    caps = dict(max_updates=ls.es.hb + 8, max_releases=16, max_tasks=tasks, max_leases=max_leases, max_renewals=1024,
                max_frees=1024, max_reports=n_servants, max_report_ids=4096)
    return ls, caps


def state(ls, caps, ticks=0):
    return SM.state_of("leased", ls, caps, ticks)


def entries(case, expires=lambda i: FAR):
    return [(t, i % N_SERVANTS, expires(i), False) for i, t in enumerate(case.ids)]


def scrambled(seq):
    seq = list(seq)
    return [seq[i] for i in sorted(range(len(seq)), key=lambda i: (i * 7919 + 13) % 1009)]


def granted(r):
    return r["task_id"][r["out"] < M.IDX_ENV_NOT_FOUND].tolist()


class ModelDriver:
    """The scripts through the model alone."""

    def __init__(self, ls, caps):
        self.ls, self.T, self.caps, self.t = ls, ls.table, dict(caps), 0
        self.seen = dict.fromkeys(("renewed", "renew_refused", "freed", "ignored_frees", "expired", "swept", "granted"), 0)

    def event(self, ips=False, **kw):
        ev = lcases.scripted(self.ls, self.ls.next_tick(), **kw)
        if ips:  # a requestor of its own per request: the inspection records differ
            ev["tasks"]["requestor_ip"] = (0x0B000000 + np.arange(len(ev["lease_expires_at"]))).astype(np.uint32)
        return ev

    def play(self, ev):
        return M.model_tick(self.ls, ev)

    def tick(self, **kw):
        r = self.play(self.event(**kw))
        self.t += 1
        for k in self.seen:
            self.seen[k] += int(r["renewed"].sum()) if k == "renewed" else len(granted(r)) if k == "granted" else r[k]
        return r

    def reserve(self, max_leases):
        self.T.max_leases = self.caps["max_leases"] = max_leases

    def remove(self, removed):
        from tests.test_stream_lease_gpu import drop_rows
        drop_rows(self.ls, np.asarray(removed, np.uint32))

    def fork(self):
        pass

    def base(self):
        pass

    def delta(self):
        pass

    def only(self, who):
        pass


# ---- the scripts (the numbers are those of tests/test_lease_table_gpu.py's docstring) ----

def found_at_every_displacement(d, case):
    """1. Every member renewed in a scrambled order, with one duplicate, one id above next_id and one
    non-member of the same home; then one servant reports half of its ids and the non-member."""
    T = d.T
    ren = [(t, 5000 + i) for i, t in enumerate(scrambled(case.ids))]
    dup = ren[0][0]
    ren = ren[:len(ren) // 2 + 1] + [(NEXT_ID + 3, 1), (dup, 77), (case.spare, 1)] + ren[len(ren) // 2 + 1:]
    r = d.tick(renew=ren)
    assert int(r["renewed"].sum()) == case.n + 1 and r["renew_refused"] == 2
    assert list(r["renewed"][[a for a, (t, _) in enumerate(ren) if t in (NEXT_ID + 3, case.spare)]]) == [0, 0]
    last = max(a for a, (t, _) in enumerate(ren) if t == dup)
    assert T.L[dup][1] == ren[last][1], "the last renewal in array order wins"
    s = T.L[case.ids[-1]][0]
    mine = lcases.held(T)[s]
    listed = mine[::2] + [case.spare]
    r = d.tick(reports=[(s, listed)])
    assert list(r["report_unknown"]) == [0] * (len(listed) - 1) + [1] and r["swept"] == 0 and r["n_leases"] == case.n


def holes_inside_the_chain(d, case):
    """2 and 3. Every other member freed; the rest renewed, reported and found behind the holes, a second
    free of a freed id ignored; a burst of grants whose ids fall in front of the holes takes them
    again; every old and new id renewed, then freed by id."""
    T = d.T
    gone, rest = case.ids[1::2], case.ids[0::2]
    r = d.tick(free=scrambled(gone))
    assert r["freed"] == len(gone) and r["n_leases"] == len(rest)
    r = d.tick(renew=[(t, 6000) for t in scrambled(rest)] + [(t, 1) for t in gone[:1]], free=gone[:1] + [case.spare])
    assert int(r["renewed"].sum()) == len(rest) and r["renew_refused"] == len(gone[:1])
    assert r["freed"] == 0 and r["ignored_frees"] == len(gone[:1]) + 1
    r = d.tick(reports=lcases.every_servant_lists_everything(T))
    assert len(r["report_unknown"]) == len(rest) and not r["report_unknown"].any() and r["swept"] == 0
    if case.n >= 63:
        assert len(case.hits(GRANTS)) >= 3, "no new id falls into the run"
    r = d.tick(n=GRANTS, lease=[FAR] * GRANTS)
    new = granted(r)
    assert new == list(range(NEXT_ID, NEXT_ID + GRANTS)), "the pool did not grant the whole burst"
    everyone = scrambled(rest + new)
    r = d.tick(renew=[(t, 7000) for t in everyone])
    assert r["renewed"].all() and len(r["renewed"]) == len(rest) + GRANTS
    r = d.tick(free=everyone)
    assert r["freed"] == len(everyone) and r["n_leases"] == 0 and int(r["running"].sum()) == 0


def contended_inserts(d, case):
    """4. One tick grants 200 requests with the run in place: the new ids whose home lies inside it all walk
    to the free slots behind it in one launch. Next tick every new id and every member is renewed and
    half of the new ones are freed by id."""
    assert len(case.hits(GRANTS)) >= 20
    r = d.tick(n=GRANTS, lease=[FAR + j for j in range(GRANTS)], ips=True)
    new = granted(r)
    assert new == list(range(NEXT_ID, NEXT_ID + GRANTS))
    r = d.tick(renew=[(t, 8000) for t in scrambled(new + case.ids)], free=new[::2])
    assert r["renewed"].all() and r["freed"] == GRANTS // 2 and r["n_leases"] == case.n + GRANTS // 2
    r = d.tick(renew=[(t, 8001) for t in new])
    assert list(r["renewed"]) == [0, 1] * (GRANTS // 2)


def expiry_entries(case):
    return entries(case, lambda i: 0 if i % 2 else FAR)


def expiry_and_sweep(d, case):
    """5. Half of the members expire at 0. At now == 0 they are not overdue and renew (to 0 again); at
    now == 1 they turn zombie; then their renewal is refused and every servant's report lists every
    other zombie of its own: exactly the unlisted ones are swept; a last round of empty reports sweeps
    the rest."""
    T = d.T
    due = case.ids[1::2]
    r = d.tick(renew=[(t, 0) for t in due])
    assert r["renewed"].all() and r["expired"] == 0
    r = d.tick()
    assert r["expired"] == len(due) and r["swept"] == 0 and r["kept_zombies"] == len(due)
    zo = {}
    for t in due:
        zo.setdefault(T.L[t][0], []).append(t)
    unlisted = sum(len(z) - len(z[::2]) for z in zo.values())
    r = d.tick(renew=[(t, 50) for t in scrambled(due)], reports=[(s, z[::2]) for s, z in sorted(zo.items())])
    assert not r["renewed"].any() and r["swept"] == unlisted and r["report_unknown"].all()
    assert r["n_leases"] == case.n - unlisted
    r = d.tick(reports=[(s, []) for s in sorted(zo)])
    assert r["swept"] == len(due) - unlisted and r["n_leases"] == case.n - len(due)
    assert not any(e[2] for e in T.L.values()) and int(r["running"].sum()) == r["n_leases"]


def reserve_with_a_chain(d, case):
    """6. Two holes, then the table is filed again into 2048 slots; every id renews, a burst is granted,
    every id is freed."""
    gone = case.ids[5:7]
    r = d.tick(free=gone)
    assert r["freed"] == 2
    d.reserve(1024)
    rest = [t for t in case.ids if t not in gone]
    r = d.tick(renew=[(t, 9000 + i) for i, t in enumerate(scrambled(rest))] + [(case.spare, 1)])
    assert int(r["renewed"].sum()) == len(rest) and r["renew_refused"] == 1
    r = d.tick(n=GRANTS, lease=[FAR] * GRANTS, ips=True)
    new = granted(r)
    assert len(new) == GRANTS
    r = d.tick(free=scrambled(rest + new))
    assert r["freed"] == len(rest) + GRANTS and r["n_leases"] == 0


def snapshot_and_restore(d, case):
    """7. The C-written snapshot of the chain state restored into a second context; both answer three
    ticks: find all, free half, grant into the run."""
    d.fork()
    r = d.tick(renew=[(t, 4000) for t in scrambled(case.ids)] + [(case.spare, 1)])
    assert int(r["renewed"].sum()) == case.n and r["renew_refused"] == 1
    r = d.tick(free=case.ids[1::2])
    assert r["freed"] == case.n // 2
    assert len(case.hits(GRANTS)) >= 20
    r = d.tick(n=GRANTS, lease=[FAR] * GRANTS)
    assert len(granted(r)) == GRANTS
    r = d.tick(renew=[(t, 4001) for t in sorted(d.T.L)])
    assert r["renewed"].all()


def delta_entries(case):
    return entries(case, lambda i: 0 if i in (0, 2) else FAR)


def delta_to_a_standby(d, case):
    """8. A first delta carries 64 grants into the intact run: where chains touch, some of them are filed
    past the bound the standby's table was loaded with, so the standby's own insert has to move it. The
    second delta's tick frees alternate members and a third of the new ids, renews others, lets two
    members expire and grants 30 more into the holes. Then the standby alone renews and frees every id."""
    T = d.T
    d.base()
    assert len(case.hits(64)) >= 8
    assert len(case.past_bound(64)) >= 3 or len(case.chains) == 1, "no insert of the delta moves the standby's bound"
    r = d.tick(n=64, lease=[FAR] * 64, ips=True)
    new = granted(r)
    assert len(new) == 64 and r["expired"] == 0
    d.delta()
    r = d.tick(free=case.ids[1::2] + new[::3], renew=[(t, 3000) for t in case.ids[4::4] + new[1::3]], n=30,
               lease=[FAR] * 30, ips=True)
    assert r["freed"] == case.n // 2 + len(new[::3]) and r["renewed"].all() and r["expired"] == 2
    assert len(granted(r)) == 30
    d.delta()
    d.only("standby")
    everyone = scrambled(sorted(T.L))
    r = d.tick(renew=[(t, 3002) for t in everyone])
    assert r["renew_refused"] == 2 and int(r["renewed"].sum()) == len(everyone) - 2
    r = d.tick(free=everyone)
    assert r["freed"] == len(everyone) and r["n_leases"] == 0 and int(r["running"].sum()) == 0


def remove_servants_with_a_chain(d, case):
    """9. Three rows leave: their members vanish from the middle of the chain; the rest are found and
    follow the compaction."""
    T = d.T
    removed = sorted({T.L[case.ids[k]][0] for k in (case.n // 2, case.n // 2 + 1, case.n // 3)})
    lost = [t for t in case.ids if T.L[t][0] in removed]
    assert len(removed) == 3 and len(lost) >= 12 and any(T.L[t][0] > removed[-1] for t in case.ids)
    d.remove(removed)
    rest = [t for t in case.ids if t not in lost]
    assert sorted(T.L) == rest
    r = d.tick(renew=[(t, 2000) for t in scrambled(case.ids)])
    assert int(r["renewed"].sum()) == len(rest) and r["renew_refused"] == len(lost)
    s = max(e[0] for e in T.L.values())
    mine = lcases.held(T)[s]
    r = d.tick(reports=[(s, mine + lost[:2])])
    assert list(r["report_unknown"]) == [0] * len(mine) + [1, 1]
    r = d.tick(n=GRANTS, lease=[FAR] * GRANTS)
    assert len(granted(r)) == GRANTS
    r = d.tick(free=sorted(T.L))
    assert r["n_leases"] == 0 and int(r["running"].sum()) == 0


# (script, the entries it starts from, the shapes it is played on)
SCRIPTS = [
    (found_at_every_displacement, entries, SHAPES),
    (holes_inside_the_chain, entries, SHAPES),
    (contended_inserts, entries, LONG),
    (expiry_and_sweep, expiry_entries, SHAPES),
    (reserve_with_a_chain, entries, [WHOLE_2048, SPLIT_2048]),
    (snapshot_and_restore, entries, [BY_NAME["wrap3_257"], TOUCHING]),
    (delta_to_a_standby, delta_entries, [BY_NAME["wrap3_257"], TOUCHING, TOUCHING_MID]),
    (remove_servants_with_a_chain, entries, [BY_NAME["wrap3_257"], TOUCHING_MID]),
]
