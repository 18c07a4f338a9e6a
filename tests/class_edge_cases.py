"""Pools made for the many-class matching kernels, and a restatement of the plan.

Which kernel places a batch is decided by a dozen hard thresholds on the registry (plan_batch and
run_planned_batch in ydc_api.hip, HostTables::build in host_tables.h): the number of servant
classes C = distinct (environment set, version) among the servants that take tasks, the number
of distinct versions V, the size and the longest row of the eligible-class table, the slot bound,
and two LDS budgets. The synthetic pools land "somewhere above 256 classes"; class_pool(C, ...)
lands ON a class count, a row length, a version count and a slot bound:

  classes      class i advertises the pair of digests {i mod E, (i mod E + 1 + i div E) mod E}
               (distinct pairs, every digest in at most 64 classes: "sparse") and the version
               vers[i mod V];
  row_lens     one more digest per entry, advertised by exactly that many classes (0: by nobody —
               an empty row; > 64: the registry is "dense" and leaves k_walk_groups);
  ballast      servants of class 0 with huge num_processors == max_tasks and running_tasks 30
               below them: they raise the slot bound (sum of min(max_tasks, nproc)) by an exact
               amount, not the free slots, and stay below 2^21 each (exact sort keys).

plan_of(sv, n_tasks) restates what the planner derives from a registry. The constants are
RESTATED here, not read from the headers: when a threshold moves, these tests fail and somebody
looks. commit_cases() are hand-made blocks of 64 requests for the commit rule of k_walk_groups
(wide_kernel.h). No GPU code in this file."""
import functools

import numpy as np

from yadcc_amd import synth

GIB = 1 << 30
FOREIGN = 0xAC100001  # 172.16.0.1: nobody's host
UNKNOWN_ENV = 0xFFFF
ENF, TIMEOUT = 0xFFFFFFFE, 0xFFFFFFFF

# ---- the planner's constants, restated ---------------------------------------------------------
MAX_FUSED_CLASSES = 8         # kernels.h kMaxFusedClasses
MAX_WAVE_CLASSES = 256        # dispatch_core.h kMaxWaveClasses
MAX_WIDE_CLASSES = 3072       # wide_kernel.h kMaxWideClasses
TICK_MAX_CLASSES = 4096       # tick_kernel.h kTickMaxClasses
GROUP_WALK_MAX_LDS = 160 * 1024 - 512  # wide_kernel.h kGroupWalkMaxLds
ELIG_MAX_VERSIONS = 16        # host_tables.h: V <= 16
ELIG_MAX_WORDS = 1 << 20      # host_tables.h: 64 EW (V + 1) ceil(C / 64) <= 2^20
WALK_MAX_ROW = 64             # plan_batch: elig_max_len <= 64
BALLAST_MAX = (1 << 21) - 1   # one servant's capacity while the sort key stays exact
BALLAST_FREE = 30

MATCH, WALK_PACKED, WALK_UNPACKED, WIDE, GENERIC = (
    "k_match_pass", "k_walk_groups:packed", "k_walk_groups:unpacked", "k_sim_wide", "k_sim_generic")
PATHS = (MATCH, WALK_PACKED, WALK_UNPACKED, WIDE, GENERIC)


def wide_lds_bytes(C):
    W = (C + 63) // 64
    W8 = (W + 7) & ~7
    return 7 * C * 4 + 2 * W8 * 64 * 4 + 16 + (64 * W8 + 2 * W) * 8


def group_walk_lds_bytes(C, n_rows, n_list, packed=False):
    return (wide_lds_bytes(C) + (3 if packed else 2) * C * 4 + (8 if packed else 0) + (n_rows + 4) * 4 +
            (n_list + 8 * n_rows) * 2 + 32 + 2 * ((n_rows + 15) & ~15))


def class_table(sv):
    """(env words per class [C, EW], version per class [C]) of the servants that take tasks, in the
    order of their first appearance in the registry (the class ids of HostTables::build)."""
    mask = np.asarray(sv["env_mask"], np.uint64)
    mask = mask.reshape(len(mask), -1)
    takes = np.asarray(sv["max_tasks"]) > 0
    sig = np.concatenate([mask[takes], np.asarray(sv["version"], np.uint64)[takes, None]], axis=1)
    if len(sig) == 0:
        return mask[:0], np.zeros(0, np.uint32)
    _, first = np.unique(sig, axis=0, return_index=True)
    sig = sig[np.sort(first)]
    return sig[:, :-1], sig[:, -1].astype(np.uint32)


def plan_of(sv, n_tasks):
    """What plan_batch / run_planned_batch derive from a registry, in plain Python (one GPU, the
    default switches, a batch too large for the tick kernel)."""
    env, ver = class_table(sv)
    C, EW = len(ver), max(1, env.shape[1])
    vs = np.unique(ver)
    V = len(vs)
    W = max(1, (C + 63) // 64)
    p = dict(C=C, V=V, env_words=EW, W=W, W8=(W + 7) & ~7, n_tasks=n_tasks)
    takes = np.asarray(sv["max_tasks"]) > 0
    p["slot_bound"] = int(np.minimum(sv["max_tasks"], sv["num_processors"])[takes].astype(np.int64).sum())
    p["table_words"] = 64 * EW * (V + 1) * ((C + 63) // 64)
    p["rows_exist"] = bool(C and V <= ELIG_MAX_VERSIONS and p["table_words"] <= ELIG_MAX_WORDS)
    p["lists_exist"] = p["rows_exist"] and C > MAX_WAVE_CLASSES
    p["n_rows"] = p["n_list"] = p["elig_max_len"] = 0
    p["row_len"] = None
    if p["rows_exist"]:
        bits = (env[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
        has = bits.reshape(C, 64 * EW).astype(np.int64)              # [class, digest]
        ge = (ver[:, None] >= vs[None, :]).astype(np.int64)           # [class, version threshold]
        row_len = np.concatenate([has.T @ ge, np.zeros((64 * EW, 1), np.int64)], axis=1)  # (vi == V: none)
        p["row_len"] = row_len
        if p["lists_exist"]:
            p["n_rows"], p["n_list"], p["elig_max_len"] = int(row_len.size), int(row_len.sum()), int(row_len.max())
    cbits = 1
    while (1 << cbits) < C:
        cbits += 1
    p["walk_cbits"] = cbits
    p["match_words"] = 1 if W == 1 else 2 if W == 2 else 4
    p["init_fill_class"] = 8 if C <= 8 else 16 if C <= 16 else 0  # (plan_batch: C <= 8, C <= 16, else)
    p["fused_class_pass"] = 1 < C <= MAX_FUSED_CLASSES
    p["tick_takes_classes"] = C <= TICK_MAX_CLASSES
    p["wide_lds"] = wide_lds_bytes(C)
    p["walk_lds"] = group_walk_lds_bytes(C, p["n_rows"], p["n_list"])
    p["walk_lds_packed"] = group_walk_lds_bytes(C, p["n_rows"], p["n_list"], True)
    p["wide_lists"] = (MAX_WAVE_CLASSES < C <= MAX_WIDE_CLASSES and p["lists_exist"] and
                       p["elig_max_len"] <= WALK_MAX_ROW)
    p["group_walk"] = p["wide_lists"] and C <= 65535 and p["walk_lds"] <= GROUP_WALK_MAX_LDS
    p["packed_bits_fit"] = p["slot_bound"] + 1 < (1 << (32 - cbits))
    p["walk_packed"] = p["group_walk"] and p["packed_bits_fit"] and p["walk_lds_packed"] <= GROUP_WALK_MAX_LDS
    if C <= MAX_WAVE_CLASSES:
        p["kernel"] = MATCH
    elif C > MAX_WIDE_CLASSES:
        p["kernel"] = GENERIC
    elif p["group_walk"]:
        p["kernel"] = WALK_PACKED if p["walk_packed"] else WALK_UNPACKED
    else:
        p["kernel"] = WIDE
    return p


# ---------------------------------------------------------------------------------------------
# class_pool
# ---------------------------------------------------------------------------------------------
def pair_digests(C):
    """(E, a, b): C distinct unordered pairs {a[i], b[i]} over E digests, every digest in at most
    2 ceil(C / E) <= 64 of them. ({a, a + k} with k <= (E - 1) / 2: two of them are equal only if
    k + k' == E.)"""
    E = 3
    while -(-C // E) > (E - 1) // 2 or 2 * -(-C // E) > 64:
        E += 1
    i = np.arange(C)
    a = i % E
    return E, a, (a + 1 + i // E) % E


def family_shape(C, V=1):
    """(env_words, n_rows, n_list) of class_pool(C) with one version and no special rows — the
    sparse family the LDS boundaries are searched in — without building it."""
    E, _, _ = pair_digests(C)
    EW = (E + 1 + 63) // 64
    return EW, 64 * EW * (V + 1), 2 * C


def class_pool(C, versions=1, row_lens=(), servants_per_class=1, shared_ip_frac=0.0, oversubscribed=False,
               ballast_slots=0, n_tasks_hint=1500, env_words=None, seed=0):
    """Servant columns of a registry with exactly C classes (see the module's docstring). The
    special digests are numbered E, E + 1, ... in the order of row_lens; pool_digests(sv) names
    every digest a request may ask for."""
    assert 1 <= versions <= 17 and C >= versions and all(0 <= n <= C for n in row_lens)
    rng = np.random.default_rng(7000 + seed)
    E, a, b = pair_digests(C)
    D = E + len(row_lens)
    EW = max((D + 1 + 63) // 64, env_words or 1)  # (one digest of the mask stays nobody's)
    cls_mask = np.zeros((C, EW), np.uint64)
    one = np.uint64(1)
    for d in (a, b):
        np.bitwise_or.at(cls_mask, (np.arange(C), d // 64), one << (d % 64).astype(np.uint64))
    for j, n in enumerate(row_lens):
        who = ((j * 37) % C + np.arange(n)) % C
        cls_mask[who, (E + j) // 64] |= one << np.uint64((E + j) % 64)
    vers = 21 - versions + np.arange(versions)  # ... 19, 20
    cls_ver = vers[np.arange(C) % versions]
    S = max(C * servants_per_class, 64)
    cls = np.arange(S) % C
    mean_free = (0.5 if oversubscribed else 1.5) * n_tasks_hint / S
    nproc = rng.choice([4, 8, 12, 16, 24, 32], S) + int(2 * mean_free)
    ded = rng.random(S) < 0.3
    max_tasks = rng.integers(1, nproc + 1)
    max_tasks = np.where((np.arange(S) >= C) & (rng.random(S) < 0.03), 0, max_tasks)  # (never a class's only servant)
    load = np.where(rng.random(S) < 0.2, (rng.random(S) * nproc / 2).astype(np.int64), 0)
    free = rng.poisson(mean_free, S)
    run = np.maximum(0, max_tasks - free)
    run = np.where(rng.random(S) < 0.03, max_tasks + 2, run)  # (more running than it may: offers nothing)
    avail = np.where(rng.random(S) < 0.03, 2 * GIB, 32 * GIB)
    ip = (10 << 24) + 1 + np.arange(S, dtype=np.int64)
    port = np.full(S, 8335, np.int64)
    if shared_ip_frac > 0:
        share = np.nonzero(rng.random(S) < shared_ip_frac)[0]
        share = share[share > 0]
        ip[share] = ip[(rng.random(len(share)) * share).astype(np.int64)]
        port[share] = 8336 + np.arange(len(share))
    cols = dict(version=cls_ver[cls], num_processors=nproc, current_load=load, max_tasks=max_tasks, running_tasks=run,
                priority=np.where(ded, synth.PRIORITY_DEDICATED, synth.PRIORITY_USER), ip=ip, port=port)
    mask = cls_mask[cls]
    mem_avail = avail
    if ballast_slots:
        parts = []
        left = ballast_slots
        while left:
            take = min(left, BALLAST_MAX)
            if 0 < left - take < 64:
                take = left - 64
            parts.append(take)
            left -= take
        assert min(parts) > BALLAST_FREE, "ballast_slots too small to hide"
        nb = len(parts)
        parts = np.array(parts, np.int64)
        add = dict(version=np.full(nb, cls_ver[0]), num_processors=parts, current_load=np.zeros(nb, np.int64),
                   max_tasks=parts, running_tasks=parts - BALLAST_FREE,
                   priority=np.full(nb, synth.PRIORITY_USER), ip=(10 << 24) + (200 << 16) + np.arange(nb),
                   port=np.full(nb, 8335))
        cols = {k: np.concatenate([v, add[k]]) for k, v in cols.items()}
        mask = np.concatenate([mask, np.repeat(cls_mask[:1], nb, axis=0)])
        mem_avail = np.concatenate([mem_avail, np.full(nb, 32 * GIB)])
    sv = {k: v.astype(np.uint32) for k, v in cols.items()}
    sv["total_memory"] = np.full(len(mask), 64 * GIB, np.uint64)
    sv["memory_available"] = mem_avail.astype(np.uint64)
    sv["env_mask"] = mask[:, 0].copy() if EW == 1 else mask
    assert len(class_table(sv)[1]) == C, (C, len(class_table(sv)[1]))
    return sv


def pool_digests(sv):
    """The digests somebody advertises, ascending."""
    env, _ = class_table(sv)
    bits = (env[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return np.nonzero(bits.reshape(len(env), -1).any(axis=0))[0]


def class_tasks(sv, n, seed=0, digests=None, own_frac=0.12, unknown_frac=0.02):
    """n requests: digests somebody advertises (each about equally often), a few unknown ones (beyond
    the masks, and the highest bit of the masks, which nobody advertises), min_version on both
    sides of every version of the pool, requestors that are nobody's host and servants' own hosts
    (the shared ones among them)."""
    rng = np.random.default_rng(8000 + seed)
    d = pool_digests(sv) if digests is None else np.asarray(digests)
    env = d[rng.integers(0, len(d), n)]
    words = np.asarray(sv["env_mask"]).reshape(len(sv["version"]), -1).shape[1]
    u = rng.random(n)
    env = np.where(u < unknown_frac / 2, UNKNOWN_ENV, np.where(u < unknown_frac, 64 * words - 1, env))
    vs = np.unique(sv["version"])
    marks = np.array([0, int(vs[0]), int(vs[len(vs) // 2]), int(vs[-1]), int(vs[-1]) + 1])
    minv = marks[rng.choice(5, n, p=[0.4, 0.15, 0.2, 0.22, 0.03])]
    rip = FOREIGN + rng.integers(0, 1 << 16, n)
    own = rng.random(n) < own_frac
    rip = np.where(own, sv["ip"][rng.integers(0, len(sv["ip"]), n)].astype(np.int64), rip)
    return {"env_id": env.astype(np.uint32), "min_version": minv.astype(np.uint32),
            "requestor_ip": rip.astype(np.uint32)}


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
class Case:
    """name, kind, the path the case is made for, what it promises, and (lazily) its pool and batch."""

    def __init__(self, name, kind, path, build, **promise):
        self.name, self.kind, self.path, self._build, self.promise = name, kind, path, build, promise
        self.info = {}  # (what the builder wants to tell: the registry index of the hand-made classes)

    @functools.lru_cache(maxsize=None)
    def data(self):
        return self._build(self)

    def __repr__(self):
        return self.name


CLASS_COUNTS = (1, 8, 9, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024,
                1025, 2047, 2048, 2049, 3071, 3072, 3073, 4096, 4097)
# The sparse family (one version, rows of at most 64 classes, a few hundred rows) on the two LDS
# bounds of k_walk_groups, found by lds_boundaries() from the formulas and pinned here: W8 steps
# from 40 to 48 words behind 2560 classes, which the packed form's third array no longer fits.
LAST_PACKED_C, LAST_WALK_C = 2560, 2694
BITS_C = 1500  # walk_cbits == 11: head ranks below 2^21 - 1


def lds_boundaries():
    """(largest C whose packed walk fits the LDS, largest C whose unpacked walk fits) in the sparse
    family, from the restated formulas alone."""
    fits = {True: 0, False: 0}
    for C in range(MAX_WAVE_CLASSES + 1, MAX_WIDE_CLASSES + 1):
        _, n_rows, n_list = family_shape(C)
        for packed in (True, False):
            if group_walk_lds_bytes(C, n_rows, n_list, packed) <= GROUP_WALK_MAX_LDS:
                fits[packed] = C
    return fits[True], fits[False]


def sparse_path(C):
    """The path of the sparse family at C classes, from the pinned boundaries."""
    if C <= MAX_WAVE_CLASSES:
        return MATCH
    if C > MAX_WIDE_CLASSES:
        return GENERIC
    return WALK_PACKED if C <= LAST_PACKED_C else WALK_UNPACKED if C <= LAST_WALK_C else WIDE


def _count_case(C, dense, k):
    over = k % 2 == 1
    n = 1024 if C > MAX_WIDE_CLASSES else (1000, 1500, 2048)[k % 3]
    path = sparse_path(C) if not dense else (GENERIC if C > MAX_WIDE_CLASSES else WIDE)

    def build(case):
        sv = class_pool(C, versions=min(C, 1 + k % 3), row_lens=(65 + k % 7,) if dense else (), oversubscribed=over,
                        servants_per_class=2 if C <= 1024 else 1, shared_ip_frac=0.1, n_tasks_hint=n, seed=C + dense)
        return sv, class_tasks(sv, n, seed=C + dense)

    return Case("C%d%s" % (C, "-dense" if dense else ""), "count", path, build, C=C, oversubscribed=over,
                dense=dense, V=min(C, 1 + k % 3))


def count_cases():
    out, k = [], 0
    for C in CLASS_COUNTS:
        for dense in (False, True) if C > MAX_WAVE_CLASSES else (False,):
            out.append(_count_case(C, dense, k))
            k += 1
    return out


ROW_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64)
ROWS_C = 600


def _rows_case(name, C, path, row_lens, versions=1, env_words=None, n=1200, special_frac=0.7, **promise):
    def build(case):
        sv = class_pool(C, versions=versions, row_lens=row_lens, shared_ip_frac=0.05, n_tasks_hint=n,
                        env_words=env_words, seed=len(name) + C)
        tk = class_tasks(sv, n, seed=C + versions)
        if row_lens:  # most requests ask for the digests of the made rows, each of them often
            E = pair_digests(C)[0]
            rng = np.random.default_rng(C)
            pick = rng.random(n) < special_frac
            tk["env_id"] = np.where(pick, E + np.arange(n) % len(row_lens), tk["env_id"]).astype(np.uint32)
            tk["min_version"] = np.where(pick & (rng.random(n) < 0.8), 0, tk["min_version"]).astype(np.uint32)
        return sv, tk

    return Case(name, "rows", path, build, C=C, V=versions, row_lens=tuple(row_lens), **promise)


def rows_cases():
    # 64 EW (V + 1) ceil(C / 64) with V == 16 and 47 class words: 1 022 720 at 20 mask words,
    # 1 073 856 at 21 — on both sides of 2^20
    return [
        _rows_case("rows-every-length", ROWS_C, WALK_PACKED, ROW_LENGTHS),
        _rows_case("rows-one-of-65", ROWS_C, WIDE, ROW_LENGTHS + (65,)),
        _rows_case("V16-C200", 200, MATCH, (), versions=16, rows_exist=True),
        _rows_case("V17-C200", 200, MATCH, (), versions=17, rows_exist=False),
        _rows_case("V16-C600", 600, WALK_PACKED, (), versions=16, rows_exist=True),
        _rows_case("V17-C600", 600, WIDE, (), versions=17, rows_exist=False),
        _rows_case("table-below-2^20", 3000, WIDE, (), versions=16, env_words=20, rows_exist=True, table_words=1022720),
        _rows_case("table-above-2^20", 3000, WIDE, (), versions=16, env_words=21, rows_exist=False,
                   table_words=1073856),
    ]


def _budget_case(name, C, path, ballast=0, **promise):
    def build(case):
        sv = class_pool(C, n_tasks_hint=1200, shared_ip_frac=0.05, seed=C)
        if ballast:  # (the ballast that puts slot_bound + 1 on the value the case names)
            bound = plan_of(sv, 1200)["slot_bound"]
            sv = class_pool(C, n_tasks_hint=1200, shared_ip_frac=0.05, seed=C, ballast_slots=ballast - 1 - bound)
        return sv, class_tasks(sv, 1200, seed=C)

    return Case(name, "budget", path, build, C=C, slot_bound_plus_1=ballast or None, **promise)


def budget_cases():
    limit = 1 << (32 - 11)
    return [
        _budget_case("lds-last-packed", LAST_PACKED_C, WALK_PACKED),
        _budget_case("lds-first-unpacked", LAST_PACKED_C + 1, WALK_UNPACKED),
        _budget_case("lds-last-walk", LAST_WALK_C, WALK_UNPACKED),
        _budget_case("lds-first-wide", LAST_WALK_C + 1, WIDE),
        _budget_case("bits-last-packed", BITS_C, WALK_PACKED, ballast=limit - 1, walk_cbits=11),
        _budget_case("bits-first-unpacked", BITS_C, WALK_UNPACKED, ballast=limit, walk_cbits=11),
    ]


# ---------------------------------------------------------------------------------------------
# The commit rule of k_walk_groups: hand-made blocks of 64 requests
# ---------------------------------------------------------------------------------------------
N_FILL, FILL_FIRST = 280, 90
HOST = (10 << 24) + (2 << 16)  # hosts of the hand-made servants: 10.2.x.y


def _srv(cap, run=0, ded=False, host=None, nproc=None):
    """A servant that offers the slots run .. cap - 1 (no foreign load)."""
    return dict(cap=cap, run=run, ded=ded, host=host, nproc=nproc or cap)


def _cls(digests, *servants, ver=20):
    return dict(d=tuple(digests), ver=ver, sv=list(servants))


def _req(d, rip=None, minv=0):
    return (d, minv, rip)


def _disjoint(d0, n):
    """n one-class rows and a request for each."""
    return [_cls([d0 + i], _srv(4)) for i in range(n)], [_req(d0 + i) for i in range(n)]


def sc_disjoint():
    return _disjoint(0, 64) + (dict(iters=1, commits=64, losers=0, blocked=0, gens=0, timeouts=0),)


def sc_one_class():
    cl = [_cls([0], *[_srv(20) for _ in range(4)])]
    return cl, [_req(0)] * 64, dict(iters=64, commits=64, losers=2016, gens=0, timeouts=0)


def sc_dry():
    cl = [_cls([0], _srv(20), _srv(20))]
    return cl, [_req(0)] * 64, dict(iters=41, commits=40, gens=0, timeouts=24)


def sc_dry_second_choice():
    # the better class: a dedicated servant below half of its processors (tier 0) with 40 slots
    cl = [_cls([0, 1], _srv(40, ded=True, nproc=80)), _cls([0, 2], _srv(30, run=3))]
    return cl, [_req(0)] * 64, dict(commits=64, gens=0, timeouts=0, servants=[0] * 40 + [1] * 24)


def sc_short_lists():
    """Classes of 1, 2, 3 and 4 entries, each asked two times more often than it has entries, three
    times over; the rest of the block are one-class rows."""
    cl, blk, d = [], [], 0
    for _ in range(3):
        for k in (1, 2, 3, 4):
            cl.append(_cls([d], _srv(k)))
            blk += [_req(d)] * (k + 2)
            d += 1
    c2, b2 = _disjoint(d, 64 - len(blk))
    return cl + c2, blk + b2, dict(gens=0, timeouts=24, commits=40)


def _chain(d0, n, down, dup):
    """Classes K_0 .. K_n, digest d0 + i in K_i and K_i+1. down: K_j's head is better than K_j+1's
    (request i picks K_i, which request i - 1 can reach as well); else the other way round (request i
    picks K_i+1, which no earlier request can reach). dup: the first request twice — the second of
    them loses its claim, marks its row, and the marks run down the block."""
    cl = []
    for j in range(n + 1):
        ds = [d0 + x for x in (j - 1, j) if 0 <= x < n]
        cl.append(_cls(ds, _srv(200, run=j if down else n + 6 - j)))
    blk = [_req(d0 + i) for i in range(n)]
    if dup:
        blk = [blk[0]] + blk[:-1]
    return cl, blk


def sc_chain():
    """Marks start from a lane that LOST a claim (wide_kernel.h: `mark = loser`), so a chain needs one:
    lanes 0 and 1 ask alike, lane 1 loses and marks K_0 and K_1, lane 2's pick K_1 carries an earlier
    lane's mark, lane 2 marks K_2, ... to the end of the block. (With the heads the other way round —
    sc_chain_up — every request picks a class no earlier request can reach: nobody waits.)"""
    cl, blk = _chain(0, 64, True, True)
    return cl, blk, dict(gens=0, timeouts=0, blocked_some=True, iters_more_than=1)


def sc_chain_up():
    cl, blk = _chain(0, 64, False, False)
    return cl, blk, dict(gens=0, timeouts=0, iters=1, commits=64, losers=0, blocked=0)


def _barrier(lanes):
    """Class B (digest 0): the servant of host 1 at its head, 90 slots of somebody else behind. The
    requests in `lanes` come from host 1."""
    cl = [_cls([0], _srv(50, host=1), _srv(100, run=10))]
    c2, b2 = _disjoint(1, 64)
    blk = [_req(0, rip=HOST + 1) if i in lanes else b2[i] for i in range(64)]
    return cl + c2, blk, dict(gens=len(lanes), timeouts=0, commits=64 - len(lanes), barrier_lanes=tuple(lanes))


def sc_barrier_lane0():
    return _barrier((0,))


def sc_barrier_lane63():
    return _barrier((63,))


def sc_barrier_adjacent():
    return _barrier((31, 32))


def sc_barrier_all():
    return _barrier(tuple(range(64)))


def sc_holes():
    """Lane 5 comes from host 1 and steps over its own servant's slot at the head of B; lanes 20 and
    40 (nobody's hosts) ask for digest 1, whose row is {B, B2}: B has holes, and the hole is theirs."""
    cl = [_cls([0, 1], _srv(50, host=1), _srv(100, run=10)), _cls([1, 2], _srv(10, run=5))]
    c2, b2 = _disjoint(3, 64)
    blk = list(b2)
    blk[5] = _req(0, rip=HOST + 1)
    blk[20] = blk[40] = _req(1)
    return cl + c2, blk, dict(timeouts=0, gens_at_least=2)


def sc_self_shared():
    """Host 1 runs two servants, in two classes of one row."""
    cl = [_cls([0, 1], _srv(10, host=1)), _cls([0, 2], _srv(10, run=1, host=1)), _cls([0, 3], _srv(10, run=2))]
    c2, b2 = _disjoint(4, 64)
    blk = list(b2)
    for lane in (3, 4, 30, 63):
        blk[lane] = _req(0, rip=HOST + 1)
    return cl + c2, blk, dict(timeouts=0, gens_at_least=4)


def _shift(cl, blk, d0, h0):
    cl = [dict(c, d=tuple(d0 + x for x in c["d"]),
               sv=[dict(s, host=None if s["host"] is None else s["host"] + h0) for s in c["sv"]]) for c in cl]
    blk = [(d + d0 if d < UNKNOWN_ENV else d, mv, None if rip is None else rip + h0) for d, mv, rip in blk]
    return cl, blk


def sc_finals():
    """Pieces of everything above, and in every fourth lane a request that is final the moment it
    is seen: an unknown digest, a min_version nobody has, a digest nobody advertises, a class
    without a free slot."""
    cl, blk, d, h = [], [], 0, 0

    def add(c, b, nd, nh=0):
        nonlocal d, h
        c, b = _shift(c, b, d, h)
        cl.extend(c)
        blk.extend(b)
        d += nd
        h += nh

    add([_cls([0], _srv(5))], [_req(0)] * 8, 1)                       # runs dry after five
    add(*_disjoint(0, 6), 6)
    add(*_chain(0, 8, True, True), 8)
    add([_cls([0, 1], _srv(50, host=1), _srv(100, run=10)), _cls([1, 2], _srv(10, run=5))],
        [_req(2), _req(0, rip=HOST + 1), _req(1), _req(1), _req(0, rip=HOST + 1)], 3, 1)
    add([_cls([0, 1], _srv(10, host=1)), _cls([0, 2], _srv(10, run=1, host=1))],
        [_req(0, rip=HOST + 1), _req(0), _req(0, rip=HOST + 1)], 3, 1)
    for k in (1, 2, 3):
        add([_cls([0], _srv(k))], [_req(0)] * (k + 1), 1)
    full = d
    cl.append(_cls([full], _srv(4, run=4)))                            # takes tasks, offers none
    d += 1
    nobody = d                                                         # (a digest of the masks nobody has)
    d += 1
    add(*_disjoint(0, 48 - len(blk)), 48 - len(blk))
    finals = [_req(UNKNOWN_ENV), _req(full), _req(0, minv=99), _req(nobody)]
    out = []
    for i in range(64):
        out.append(finals[(i // 4) % 4] if i % 4 == 3 else blk.pop(0))
    assert not blk
    return cl, out, dict(finals=16)


SCENARIOS = (sc_disjoint, sc_one_class, sc_dry, sc_dry_second_choice, sc_short_lists, sc_chain, sc_chain_up,
             sc_barrier_lane0, sc_barrier_lane63, sc_barrier_adjacent, sc_barrier_all, sc_holes, sc_self_shared,
             sc_finals)
COMMIT_SIZES = (64, 65, 127, 128)


def hand_pool(classes):
    """The registry of a scenario: N_FILL filler classes (pairs of filler digests, one servant of
    four slots each) around the hand-made ones, more than 256 classes in all and every row far
    below 64. Returns (servant columns, first registry index of every hand-made class, the filler
    digests)."""
    H = 1 + max(max(c["d"]) for c in classes) + 1  # (+ 1: sc_finals' digest nobody advertises)
    E, a, b = pair_digests(N_FILL)
    EW = (H + E + 1 + 63) // 64
    one = np.uint64(1)  # (rows below: mask words, version, nproc, max_tasks, running, dedicated, ip)

    def mask_of(digests):
        m = np.zeros(EW, np.uint64)
        for x in digests:
            m[x // 64] |= one << np.uint64(x % 64)
        return m

    fill = [(mask_of((H + int(a[i]), H + int(b[i]))), 20, 8, 4, i % 3, False, (10 << 24) + (1 << 16) + i)
            for i in range(N_FILL)]
    hand, first = [], []
    for c in classes:
        first.append(FILL_FIRST + len(hand))
        for s in c["sv"]:
            ip = HOST + s["host"] if s["host"] is not None else (10 << 24) + (3 << 16) + len(hand)
            hand.append((mask_of(c["d"]), c["ver"], s["nproc"], s["cap"], s["run"], s["ded"], ip))
    rows = fill[:FILL_FIRST] + hand + fill[FILL_FIRST:]
    S = len(rows)
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    ip = col(6, np.uint32)
    port = np.full(S, 8335, np.uint32)
    seen = {}
    for s in range(S):  # (a host's servants: one port each)
        port[s] += seen.get(int(ip[s]), 0)
        seen[int(ip[s])] = seen.get(int(ip[s]), 0) + 1
    mask = np.stack([r[0] for r in rows])
    sv = {"version": col(1, np.uint32), "num_processors": col(2, np.uint32), "current_load": np.zeros(S, np.uint32),
          "max_tasks": col(3, np.uint32), "running_tasks": col(4, np.uint32),
          "priority": np.where(col(5, bool), synth.PRIORITY_DEDICATED, synth.PRIORITY_USER).astype(np.uint32),
          "total_memory": np.full(S, 64 * GIB, np.uint64), "memory_available": np.full(S, 32 * GIB, np.uint64),
          "env_mask": mask[:, 0].copy() if EW == 1 else mask, "ip": ip, "port": port}
    assert len(class_table(sv)[1]) == N_FILL + len(classes) > MAX_WAVE_CLASSES
    return sv, first, H + np.arange(E)


def _columns(reqs):
    return {"env_id": np.array([d for d, _, _ in reqs], np.uint32),
            "min_version": np.array([mv for _, mv, _ in reqs], np.uint32),
            "requestor_ip": np.array([FOREIGN + i if rip is None else rip for i, (_, _, rip) in enumerate(reqs)],
                                     np.uint32)}


def _commit_case(sc, size):
    def build(case):
        classes, block, _ = sc()
        assert len(block) == 64
        sv, first, fill_digests = hand_pool(classes)
        case.info["first"] = first
        blk = _columns(block)
        # the random block: filler digests only (the hand-made classes are untouched when their
        # block comes second), a fifth of it from the filler servants' own hosts
        rnd = class_tasks(sv, 64, seed=size, digests=fill_digests, own_frac=0.0, unknown_frac=0.05)
        rng = np.random.default_rng(size)
        own = rng.random(64) < 0.2
        fill_ip = (10 << 24) + (1 << 16) + rng.integers(0, N_FILL, 64)
        rnd["requestor_ip"] = np.where(own, fill_ip, rnd["requestor_ip"]).astype(np.uint32)
        parts = {64: [blk], 65: [blk, {k: v[:1] for k, v in rnd.items()}],
                 127: [rnd, {k: v[:63] for k, v in blk.items()}], 128: [rnd, blk]}[size]
        tk = {k: np.concatenate([p[k] for p in parts]) for k in blk}
        return sv, tk

    promise = sc()[2]
    return Case("%s-%d" % (sc.__name__[3:], size), "commit", WALK_PACKED, build, size=size,
                block_at=0 if size <= 65 else 64, block_len=63 if size == 127 else 64, scenario=sc.__name__[3:],
                **promise)


def commit_cases():
    return [_commit_case(sc, size) for sc in SCENARIOS for size in COMMIT_SIZES]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(count_cases() + rows_cases() + budget_cases() + commit_cases())


def case(name):
    return {c.name: c for c in all_cases()}[name]
