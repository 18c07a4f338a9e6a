"""Crafted inputs for the usage table (yadcc_amd/csrc/stream_usage.h) and their expectations in plain
Python integers: requestor ids that share a home slot of the table, rows of W whose counts need the
upper half of a 32-bit lane value, lease tables whose every lease lies in a slot the test chose, and
the sizes at which the host's bound makes the table grow. One list of inputs, used two ways:
tests/test_usage_table_model.py rehearses them on the CPU (the chains form, the leases lie where the
patterns say, the closed forms add up), tests/test_usage_table_gpu.py feeds them to the kernels.

Nothing here calls the library. The hash is tests/hash_index_cases.py's restatement (mix, ip_colliders,
one_chain, layout, run_of, absent_around), the lease slot tests/lease_table_cases.py's (home, colliders,
layout). An expectation is an Expect: requestor -> five sums modulo 2^64, built from the crafted list
itself: a lease charges dq to its requestor's slot_time (and zombie_time, prefetch_time as its flags
say), a lease without details charges unattributed_time, an entry of W charges dq to wait_time and
rows x dq to wait_row_time; a tick with dq == 0 files nothing and still counts.

Geometry of the accrual over L (k_usage_accrue): thread t of a workgroup owns slots 4t .. 4t + 3, wave w
owns slots 256w .. 256w + 255, a workgroup 1024 slots. A thread merges its four slots by requestor into
groups in the order it meets them; the wave combines equal first groups and hands that key (the lead)
to the workgroup, whose thread 0 merges the four waves' leads. thread_groups() and wave_lead() restate
that for a plan, so that a test can say which thread, wave and workgroup sees what.
"""
import numpy as np

from tests import hash_index_cases as H
from tests import lease_table_cases as LT
from tests import stream_usage_model as U

M64 = U.M64
BITS = H.FLOOR_BITS
SIZE = 1 << BITS
COLS = 5
FAR = LT.FAR
ROUNDS = 4  # kRequestorRounds: distinct keys a wave combines before its lanes add for themselves


# ---- the expectation --------------------------------------------------------------------------------

class Expect:
    """The table and its totals as plain integers. quantum, last: the clock of usage_quanta.h (last None:
    no tick yet, so the first tick's dq is 0)."""

    def __init__(self, quantum=1):
        self.quantum, self.last = int(quantum), None
        self.rows = {}
        self.unattributed = self.quanta = self.ticks = 0

    def dq_at(self, now):
        last = now if self.last is None else self.last
        return (int(now) // self.quantum - int(last) // self.quantum) & M64

    def add(self, ip, col, v):
        row = self.rows.setdefault(int(ip), [0] * COLS)
        row[col] = (row[col] + int(v)) & M64

    def tick(self, now, leases=(), waiting=()):
        """A tick at `now` over L = [(requestor or None, zombie, prefetch)] and W = [(requestor, rows)] as
        they are BEFORE the tick. -> dq."""
        dq = self.dq_at(now)
        if dq:
            for ip, z, p in leases:
                if ip is None:
                    self.unattributed = (self.unattributed + dq) & M64
                    continue
                self.add(ip, 0, dq)
                self.add(ip, 1, dq if z else 0)
                self.add(ip, 2, dq if p else 0)
            for ip, rows in waiting:
                self.add(ip, 3, dq)
                self.add(ip, 4, int(rows) * dq)
        self.quanta = (self.quanta + dq) & M64
        self.ticks += 1
        self.last = int(now)
        return dq

    def load(self, rows, totals=None):
        """rows: [(requestor, v0 .. v4)]; duplicates add, a row of zeros files its key."""
        for r in rows:
            for k in range(COLS):
                self.add(r[0], k, r[1 + k])
        for k, v in (totals or {}).items():
            name = {"unattributed_time": "unattributed"}.get(k, k)
            setattr(self, name, (getattr(self, name) + int(v)) & M64)

    def reset(self):
        self.rows = {}
        self.unattributed = self.quanta = self.ticks = 0

    def totals(self):
        return {"unattributed_time": self.unattributed, "quanta": self.quanta, "ticks": self.ticks, "n_keys": len(self.rows)}

    def get(self):
        out = np.zeros(len(self.rows), U.DTYPE)
        for i, ip in enumerate(sorted(self.rows)):
            out[i] = (ip, 0) + tuple(self.rows[ip])
        return out, self.totals()

    def find(self, ips):
        out = np.zeros(len(ips), U.DTYPE)
        for i, ip in enumerate(int(x) for x in ips):
            out[i] = (ip, 0) + tuple(self.rows.get(ip, [0] * COLS))
        return out


def as_rows(rows):
    """[(requestor, v0 .. v4)] -> an array of ydc_usage_row."""
    out = np.zeros(len(rows), U.DTYPE)
    for i, r in enumerate(rows):
        out[i] = (int(r[0]), 0) + tuple(int(v) for v in r[1:])
    return out


# ---- A. chains ---------------------------------------------------------------------------------------

# Odd multipliers, one per column: (i + 1) * P mod 2^64 is never 0, and the columns of one row differ.
_P = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63)


def sums_for(ids, salt=0):
    """[(id, five distinct non-zero sums)]: a row per id, every column of every row its own number."""
    out = []
    for i, ip in enumerate(ids):
        out.append((int(ip),) + tuple(((i + 1 + 1000 * salt) * p) & M64 for p in _P))
    return out


def chain(h, n, bits=BITS, kind="any", skip=()):
    """n ids of home h at `bits` that form one run from it (asserted)."""
    ids = H.ip_colliders(bits, h, n, kind=kind, skip=skip)
    H.one_chain(ids, bits, h)
    return ids


def permuted(seq, seed):
    seq = list(seq)
    return [seq[i] for i in np.random.default_rng(seed).permutation(len(seq))]


def ends():
    """0 (home 0) and 0xFFFFFFFF, each amid 63 other ids of its home: two chains that do not touch."""
    hf = H.home(0xFFFFFFFF, BITS)
    zero, ones = [0] + H.ip_colliders(BITS, 0, 63), [0xFFFFFFFF] + H.ip_colliders(BITS, hf, 63)
    H.one_chain(zero, BITS, 0)
    H.one_chain(ones, BITS, hf)
    assert H.layout(zero + ones, BITS)[0] == H.run_of(0, 64, BITS) | H.run_of(hf, 64, BITS) and 64 < hf < SIZE - 64
    return zero, ones, hf


def touching():
    """40 ids of home 1021, whose run goes on through slots 0 .. 36, and 40 of home 0: one run of 80."""
    a, b = H.ip_colliders(BITS, 1021, 56), H.ip_colliders(BITS, 0, 56)
    for col in (a[:40] + b[:40], b[:40] + a[:40]):
        occ, md = H.layout(col, BITS)
        assert occ == H.run_of(1021, 80, BITS) and md > 39, "not one run longer than either chain"
    absent = a[40:] + b[40:] + H.ip_colliders(BITS, (1021 + 80) % SIZE, 1)
    return a[:40], b[:40], absent


def doubled(h, kind, n=257):
    """n ids of home h at 1024 slots; where they lie at 2048: {home: count}."""
    ids = chain(h, n, kind=kind)
    homes = {}
    for ip in ids:
        hh = H.home(ip, BITS + 1)
        homes[hh] = homes.get(hh, 0) + 1
    want = {"stay0": {h: n}, "stay1": {h + SIZE: n}, "split": {h: (n + 1) // 2, h + SIZE: n // 2}}[kind]
    assert homes == want, (kind, homes)
    return ids, homes


def further_keys(k, skip):
    """k sequential-looking ids that are none of `skip` (the keys whose load makes the table grow)."""
    out, at, skip = [], 0x0D000000, set(int(s) for s in skip)
    while len(out) < k:
        if at not in skip:
            out.append(at)
        at += 7
    return out


def fold_chains():
    """Three chains of 65 in a 2048-slot table: one whose run crosses the tile boundary 1023 -> 1024, one
    whose run crosses the wrap 2047 -> 0, one that does neither."""
    bits = BITS + 1
    out = [chain(h, 65, bits=bits) for h in (1021, 2045, 300)]
    occ, _ = H.layout(out[0] + out[1] + out[2], bits)
    assert occ == H.run_of(1021, 65, bits) | H.run_of(2045, 65, bits) | H.run_of(300, 65, bits) and len(occ) == 195
    assert {1023, 1024} <= H.run_of(1021, 65, bits) and {2047, 0} <= H.run_of(2045, 65, bits)
    return out


# ---- B. counts that need the upper half ------------------------------------------------------------

WIDE_ROWS = (65535, 65536, 65537, 131071, 1)  # n_immediate + n_prefetch of the heavy requestor's entries
WIDE_LANES = (0, 13, 31, 32, 63)             # their positions in W (one wave: position i is lane i)
HEAVY, LIGHT = 0x0C00B001, 0x0C00B002


def wide_wave():
    """One wave of W: [(requestor, n_immediate, n_prefetch)] by queue position. The heavy requestor's five
    entries carry WIDE_ROWS, the other 59 positions are the light requestor's with one row each."""
    out = [(LIGHT, 1, 0)] * 64
    for lane, rows in zip(WIDE_LANES, WIDE_ROWS):
        out[lane] = (HEAVY, rows - 1, 1) if rows == 65537 else (HEAVY, 1, rows - 1)
    assert sum(r & 0xFFFF for r in WIDE_ROWS) >> 16 and all(r >> 16 for r in WIDE_ROWS[1:4])
    return out


# ---- C. leases at exact slots ----------------------------------------------------------------------

class Lease:
    """What a test puts into one slot of L. ip None: no details (started_at == NO_TIME)."""

    def __init__(self, ip, zombie=False, prefetch=False):
        self.ip, self.zombie, self.prefetch = (None if ip is None else int(ip)), bool(zombie), bool(prefetch)

    def triple(self):
        return (self.ip, self.zombie, self.prefetch)


def slots_of(t, wg=0):
    """The four slots of thread t of workgroup wg."""
    return [1024 * wg + 4 * t + k for k in range(4)]


def exact_ids(bits, slots):
    """One lease id per slot, alone in its home: slot == home, displacement 0 (asserted)."""
    slots = list(slots)
    ids = [LT.colliders(bits, s, 1)[0] for s in slots]
    assert len(set(ids)) == len(ids) and [LT.home(t, bits) for t in ids] == slots
    occ, md = LT.layout(ids, bits)
    assert occ == frozenset(slots) and md == 0
    return ids


def exact_stream(plan, bits=BITS):
    """plan: {slot: Lease}. -> (the model's stream, its bounds, {slot: id}): a leased stream whose table,
    once restored, holds every lease in the slot the plan names. A zombie-to-be expires at 0: the first
    tick (at now >= 1) turns it."""
    slots = sorted(plan)
    ids = exact_ids(bits, slots)
    entries = [(tid, i % LT.N_SERVANTS, 0 if plan[s].zombie else FAR, False) for i, (s, tid) in enumerate(zip(slots, ids))]
    ls, caps = LT.crafted_stream(entries, max_leases=1 << (bits - 1))
    assert LT.cap_bits(caps["max_leases"]) == bits
    return ls, caps, dict(zip(slots, ids))


def records(plan, at):
    """The columns ydc_stream_inspect_load takes for the plan's leases that have details."""
    slots = [s for s in sorted(plan) if plan[s].ip is not None]
    return dict(task_id=np.array([at[s] for s in slots], np.uint64), started_at=np.array([100 + s for s in slots], np.int64),
                env_id=np.zeros(len(slots), np.uint32), requestor_ip=np.array([plan[s].ip for s in slots], np.uint32),
                prefetch=np.array([plan[s].prefetch for s in slots], np.uint8))


def triples(plan):
    return [plan[s].triple() for s in sorted(plan)]


def thread_groups(plan, t, wg=0):
    """The groups thread t of workgroup wg merges its four slots into: [(requestor, leases, zombies,
    prefetched)] in the order met, and the leases without details."""
    groups, nobody = [], 0
    for s in slots_of(t, wg):
        le = plan.get(s)
        if le is None:
            continue
        if le.ip is None:
            nobody += 1
            continue
        for g in groups:
            if g[0] == le.ip:
                g[1] += 1
                g[2] += le.zombie
                g[3] += le.prefetch
                break
        else:
            groups.append([le.ip, 1, int(le.zombie), int(le.prefetch)])
    return [tuple(g) for g in groups], nobody


def wave_lead(plan, w, wg=0):
    """The key of wave w's deferred first round: the first group of its lowest thread that has one, with
    the counts of every thread of the wave whose first group is that key. None: the wave has no lead."""
    first = [thread_groups(plan, 64 * w + lane, wg)[0] for lane in range(64)]
    first = [g[0] for g in first if g]
    if not first:
        return None
    ip = first[0][0]
    same = [g for g in first if g[0] == ip]
    return (ip, sum(g[1] for g in same), sum(g[2] for g in same), sum(g[3] for g in same))


KEY = {"A": 0, "B": 0x0C0000B0, "C": 0x0C0000C0, "D": 0xFFFFFFFF}  # (requestor 0 and all ones are ordinary keys)
THREAD_PATTERNS = ("AAAA", "AABB", "ABAB", "ABBA", "AABC", "ABCD", "A.A.", "...A")
THREADS = ((0, 5), (0, 64 + 9))  # (workgroup, thread): the pattern once in wave 0 and once in wave 1


def _marks(pattern):
    """(slot of the zombie, slot of the prefetch byte) within the thread: the zombie on a lease of the
    third group if there is one, else of the second, else on the last live slot; the prefetch byte on
    another lease, not of the first group where the pattern has a second, and of another group than the
    zombie's where it has a third."""
    live = [k for k, c in enumerate(pattern) if c != "."]
    order = []
    for k in live:
        if pattern[k] not in order:
            order.append(pattern[k])
    group = {k: order.index(pattern[k]) for k in live}
    want = min(2, len(order) - 1)
    zi = [k for k in live if group[k] == want][0] if want else live[-1]
    rest = [k for k in live if k != zi]
    if not rest:
        return zi, zi
    pi = min(rest, key=lambda k: (group[k] == 0, group[k] == group[zi], -k))
    return zi, pi


def thread_plan(pattern):
    """The pattern in the four slots of each of THREADS, and in the next thread a lease without details
    in front of one of A's."""
    zi, pi = _marks(pattern)
    plan = {}
    for wg, t in THREADS:
        for k, (s, c) in enumerate(zip(slots_of(t, wg), pattern)):
            if c != ".":
                plan[s] = Lease(KEY[c], zombie=k == zi, prefetch=k == pi)
        nxt = slots_of(t + 1, wg)
        plan[nxt[0]], plan[nxt[1]] = Lease(None), Lease(KEY["A"])
    return plan


HOT = 0x0C00A000
SIX = [0x0C00A100 + 16 * k for k in range(6)]


def wave_plan(distinct=None):
    """Wave 0: every thread's first group is HOT (the deferred lead), every fifth thread holds it twice, and
    the second group is one of six keys (more than the wave combines: the leftover lanes add for
    themselves), with zombies and prefetch bytes among them. Wave 1: 64 distinct first keys, `distinct`
    or sequential ids."""
    distinct = [0x0C00D000 + 3 * t for t in range(64)] if distinct is None else [int(x) for x in distinct]
    assert len(set(distinct)) == 64 and not set(distinct) & set(SIX + [HOT])
    plan = {}
    for t in range(64):
        s = slots_of(t)
        plan[s[0]] = Lease(HOT, prefetch=t % 8 == 1)
        plan[s[1]] = Lease(SIX[t % 6], zombie=t % 3 == 1, prefetch=t % 4 == 2)
        if t % 5 == 0:
            plan[s[2]] = Lease(HOT, zombie=t % 10 == 0)
        plan[slots_of(64 + t)[0]] = Lease(distinct[t], zombie=t % 7 == 3, prefetch=t % 2 == 1)
    return plan


X, Y, Z, V = 0x0C00E001, 0x0C00E002, 0x0C00E003, 0x0C00E004
LEADS = {"all equal": (X, X, X, X), "A,B,A,B": (X, Y, X, Y), "A,A,B,B": (X, X, Y, Y), "all distinct": (X, Y, Z, V),
         "only wave 3": (None, None, None, X), "wave 0 empty": (None, X, X, X)}


def leads_plan(keys):
    """Wave w's lead is keys[w] (None: the wave holds nothing): three of its threads hold it, with a second
    key of the wave's own behind it, a zombie among the lead's leases in the odd waves, a prefetch byte
    in every wave."""
    plan = {}
    for w, key in enumerate(keys):
        if key is None:
            continue
        a, b, c = slots_of(64 * w), slots_of(64 * w + 7), slots_of(64 * w + 63)
        plan[a[0]], plan[a[1]], plan[a[3]] = Lease(key), Lease(key), Lease(0x0C00F000 + w, zombie=True)
        plan[b[0]] = Lease(key, zombie=w % 2 == 1)
        for k in range(4):
            plan[c[k]] = Lease(key, prefetch=k == 2)
    return plan


ONLY_AT_THE_SEAM = 0x0C00E100


def two_workgroups_plan():
    """2048 slots, two workgroups: HOT in both halves, one key only in slots 1020 .. 1027 (the last thread of
    workgroup 0 and the first of workgroup 1)."""
    plan = {}
    for wg, threads in ((0, (0, 3, 64, 130, 200)), (1, (1, 70, 128, 255))):
        for t in threads:
            s = slots_of(t, wg)
            plan[s[0]], plan[s[1]], plan[s[3]] = Lease(HOT), Lease(HOT, prefetch=t % 2 == 0), Lease(0x0C00F100 + t, zombie=wg == 1)
    for s in range(1020, 1028):
        plan[s] = Lease(ONLY_AT_THE_SEAM, zombie=s == 1022, prefetch=s == 1025)
    return plan


# ---- D. the host's bound ---------------------------------------------------------------------------

def bound(n_keys, fresh, holders):
    """usage_bound: the keys the table has, plus those L and W can have gained since they were last claimed."""
    return n_keys + min(fresh, holders)


# Requests per tick: 256 requestors first (100 of them twice), then new ones in halving numbers, so that
# n_keys + fresh stays at or below 512 and the table on its 1024-slot floor while it fills to 500 keys.
RAMP = (356, 128, 64, 32, 16, 4)
RAMP_KEYS, RAMP_LEASES, STRANGERS = 500, 600, 520


def ramp():
    """-> per tick the requestors of its requests: 500 distinct ids in all, 600 requests."""
    ids = [0x0C100000 + 13 * i for i in range(RAMP_KEYS)]
    out, at = [], 0
    for k, n in enumerate(RAMP):
        new = n if k else 256
        out.append(ids[at:at + new] + (ids[:n - new] if k == 0 else []))
        at += new
    assert at == RAMP_KEYS and sum(len(t) for t in out) == RAMP_LEASES
    return out


def strangers():
    return [0x0C200000 + 11 * i for i in range(STRANGERS)]
