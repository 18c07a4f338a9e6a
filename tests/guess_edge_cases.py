"""Pools made for the START STATES of k_match_pass, and plain restatements of what computes them.

Everything that gives a chunk its start state is a hint — the level guesses of pass 0 in their
forms, the warm-up, the walk of the dedicated tier's end (zone_guess.h) —, the passes verify and
repair, so equality with the oracle says nothing about the hints. Two kinds of pools say more:

  exact pools   every request that is eligible for any class is eligible for every class (all
                servants advertise digest 0, all versions are >= 20, requests ask for digest 0 at
                min_version 0 or 20, or for a digest nobody has) and no requestor is a servant's host:
                consumption follows the global slot order, the level guess IS the true start state,
                and a correct device replays every chunk exactly once (YDC_DEBUG_SIM=1 counts the
                replays into stats()["chunk_sims"]). Per part of the registry when the digests are
                disjoint. exact_cases(); the `form` of a case names the branch of k_match_pass that
                computes its guesses, guess_plan() restates how the planner picks it.
  walk pools    every servant advertises digest 0 besides random others, requests ask for a random
                digest, nobody comes from a servant's host. The oracle's answer to M foreign requests
                for digest 0 is the global slot order; from it follow the class lists, T0 (the first
                slot of tier 1, by slot_tier's rule), and zone_restate(): before / tail, z_lo, z_hi,
                t_start and the cursors the walk publishes, row by row, as zone_guess.h words the
                rule. true_cursors() are the class cursors the oracle's placement implies.
                walk_cases().

The constants are RESTATED here, not read from the headers: when a threshold moves, these tests
fail and somebody looks. No GPU code in this file."""
import functools

import numpy as np

from oracle import oraclebind as O
from tests.class_edge_cases import class_table
from yadcc_amd import synth

GIB = 1 << 30
FOREIGN = 0xAC100001  # 172.16.0.1 ...: nobody's host
UNKNOWN_ENV = 0xFFFF
NOBODYS_BIT = 63      # a digest of the mask word that no servant advertises
ENF, TIMEOUT = 0xFFFFFFFE, 0xFFFFFFFF

# ---- the planner's constants, restated ---------------------------------------------------------
MAX_FUSED_CLASSES = 8     # kernels.h kMaxFusedClasses
MAX_RADIX_BITS = 11       # kernels.h kMaxRadixBits
SORT_THREADS = 256        # kernels.h kSortThreads
BINSORT_MAX_SLOTS = 600000
BIN_MAX_SERVANTS = 4096   # bin_sort.h kBinMaxServants
WARM_UP = 16              # match_kernel.h kWarmUp
ZONE_MAX_ROWS = 32        # zone_guess.h kZoneMaxChunks
ZONE_LEAD, ZONE_TRAIL, ZONE_MAX_CHUNKS = 2304, 1024, 2560
BLOCK = 64                # requests per block of the matching loop: chunk sizes are multiples of it

TABLE_FILL, TABLE, WAVE, QUARTILE_TILES, QUARTILE, ONE, INIT = (
    "level table + windows into the rings", "level table", "wave-cooperative search",
    "quartile search in one tile", "quartile search", "one class", "k_guess_init")
FORMS = (TABLE_FILL, TABLE, WAVE, QUARTILE_TILES, QUARTILE, ONE, INIT)


def _bits(x):
    b = 1
    while (1 << b) < x:
        b += 1
    return b


def guess_plan(sv, n_tasks, chunk_size, binsort=1, own_guess=1, fuse_passes=1, warm_up=0, ring_total=0,
               zone_guess=1, n_parts=1, **_):
    """What plan_batch (ydc_api.hip) derives for a batch on the wave path (one GPU, <= 256 classes,
    capacities below 2^11, a forced chunk size): the form of the level guesses, the warm-up, the
    rings, and whether the walk of the tier's end is admitted."""
    env, ver = class_table(sv)
    C = len(ver)
    W = max(1, (C + 63) // 64)
    p = dict(C=C, W=W, n_tasks=n_tasks)
    cs = (chunk_size + BLOCK - 1) // BLOCK * BLOCK  # (a forced size is rounded up to whole blocks)
    K = -(-n_tasks // cs)
    p["cs"], p["K"] = cs, K
    takes = np.asarray(sv["max_tasks"]) > 0
    cap = np.minimum(sv["max_tasks"], sv["num_processors"])[takes].astype(np.int64)
    slot_bound = int(cap.sum())
    cap_bits = 1
    while cap.max() >> cap_bits:
        cap_bits += 1
    assert cap_bits <= 11 and slot_bound <= 300000, "guess_plan restates the plan of small capacities only"
    key_bits = 2 * cap_bits + 1 + (_bits(n_parts) if n_parts > 1 else 0)
    passes = -(-key_bits // MAX_RADIX_BITS)
    bpp = -(-key_bits // passes)
    cls_bits = _bits(C)
    if 1 < C <= MAX_FUSED_CLASSES and passes >= 2:  # (choose_key_format: room for the class on the last digit)
        room = MAX_RADIX_BITS - cls_bits
        if key_bits - (passes - 1) * bpp > room:
            wide = (key_bits - room + passes - 2) // (passes - 1)
            if wide <= MAX_RADIX_BITS and wide * (passes - 1) < key_bits:
                bpp = wide
    gbits = 1
    while gbits < 32 and (slot_bound >> gbits):
        gbits += 1
    packed_class = C > 1 and gbits + cls_bits <= 32
    p["binsort"] = bool(binsort and key_bits <= 32 and 1 <= C <= 256 and 0 < slot_bound <= BINSORT_MAX_SLOTS and
                        (C == 1 or packed_class) and len(sv["version"]) <= BIN_MAX_SERVANTS)
    fused = (not p["binsort"] and 1 < C <= MAX_FUSED_CLASSES and
             key_bits - (passes - 1) * bpp + cls_bits <= MAX_RADIX_BITS)
    cls_passes = 0 if (p["binsort"] or fused or C <= 1) else -(-cls_bits // MAX_RADIX_BITS)
    p["fused_class_pass"] = fused
    sort_items = 2  # (slot_bound <= 300000)
    p["tile_tab_elems"] = SORT_THREADS * sort_items
    p["n_tiles"] = max(1, -(-slot_bound // p["tile_tab_elems"]))
    p["tile_tab"] = not p["binsort"] and cls_passes == 1 and slot_bound > 0
    p["list_p"] = p["binsort"] or cls_passes > 0 or fused
    p["own_guess"] = bool(W == 1 and own_guess)
    p["level_tab"] = p["binsort"] and n_parts <= 1
    # ---- rings
    dense = W == 1 and cs >= 256
    rt = ring_total
    if rt == 0:
        rt = 2048  # (dense: 2048 while one CU's resident waves fit, which the K of these tests never exceeds)
    else:
        rt = max(256, rt)
    while rt < 2048 and (C << 3) > rt:
        rt <<= 1
    rshift = 3
    while rshift < 10 and (C << (rshift + 1)) <= rt:
        rshift += 1
    p["ring_total"], p["ring"], p["dense"] = rt, 1 << rshift, dense
    # ---- the form of the guesses (k_match_pass, "start state")
    if not p["own_guess"]:
        form = INIT
    elif p["list_p"] and p["level_tab"] and C <= 8:
        form = TABLE_FILL if C <= 4 and (C << rshift) <= rt and (1 << rshift) >= 256 else TABLE
    elif p["list_p"] and C <= 4:
        form = WAVE
    elif p["list_p"]:
        form = QUARTILE_TILES if p["tile_tab"] else QUARTILE
    else:
        form = ONE
    p["form"] = form
    # ---- warm-up (pass 0 + 1 in one launch, own guesses, one part)
    p["fused_passes"] = bool(fuse_passes)
    p["warm"] = bool(fuse_passes and p["own_guess"] and n_parts <= 1 and cs >= 64)
    p["warm_len"] = (min(64, max(1, warm_up)) if warm_up else min(64, max(WARM_UP, cs // 8))) if p["warm"] else 0
    # With warm-ups pass 0 certifies nothing (the successor did not start from its level guess):
    # the fused launch reports two rounds; every other form certifies itself in pass 0.
    p["rounds"] = 2 if p["warm"] and K > 1 else 1
    # ---- the walk of the tier's end
    p["walk"] = bool(zone_guess and W == 1 and p["own_guess"] and p["warm"] and not p["binsort"] and key_bits <= 32 and
                     8 < C <= 64 and p["tile_tab"] and 64 <= K <= ZONE_MAX_CHUNKS and slot_bound > 0 and
                     (C << 7) <= 2 * rt)
    zshift = 8
    while zshift > 7 and (C << zshift) > 2 * rt:
        zshift -= 1
    p["zone_ring"] = 1 << zshift
    return p


# ---------------------------------------------------------------------------------------------
# Pools
# ---------------------------------------------------------------------------------------------
def _servant(rng, ded, pure=False, roomy=False):
    """One servant's (nproc, load, max_tasks, running): a few free slots, sometimes foreign load, a
    dedicated one `pure` when it offers nothing at or above half of its processors (tier 0 only)."""
    nproc = int(rng.choice([8, 12, 16, 24, 32, 48]))
    max_tasks = int(rng.integers(max(1, nproc // 4), nproc + 1))
    if pure:
        max_tasks = min(max_tasks, (nproc + 1) // 2)
    load = int(rng.random() * nproc / 2) if rng.random() < 0.2 else 0
    top = min(max_tasks, nproc)
    free = top if roomy else min(top, 1 + int(rng.poisson(top / 2)))
    return nproc, load, max_tasks, top - free


def _slots(nproc, load, max_tasks, running, ded):
    """(free slots, those of tier 0) — servant_slot_count and slot_tier (dispatch_core.h)."""
    top = min(max_tasks, nproc)
    n = top - running if (max_tasks and load < nproc and running < top) else 0
    t = 0
    if ded and n:
        half = (nproc + 1) // 2  # first r with 2 r >= nproc
        t = max(0, min(top, half) - running)
    return n, t


def _columns(rows, cls_mask, cls_ver, rng, low_memory=True):
    """Servant columns of rows (class, nproc, load, max_tasks, running, dedicated), shuffled."""
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    S = len(rows)
    col = lambda k: np.array([r[k] for r in rows], np.int64)
    cls = col(0)
    sv = {"version": cls_ver[cls], "num_processors": col(1), "current_load": col(2), "max_tasks": col(3),
          "running_tasks": col(4), "priority": np.where(col(5) != 0, synth.PRIORITY_DEDICATED, synth.PRIORITY_USER),
          "ip": (10 << 24) + 1 + np.arange(S), "port": np.full(S, 8335)}
    sv = {k: np.asarray(v).astype(np.uint32) for k, v in sv.items()}
    sv["total_memory"] = np.full(S, 64 * GIB, np.uint64)
    sv["memory_available"] = np.full(S, 32 * GIB, np.uint64)
    sv["env_mask"] = cls_mask[cls].astype(np.uint64)
    return sv


def classes_with_digest0(C, versions=1, first_version=20):
    """C classes that all advertise digest 0: class i has the other bits of i // versions (digests
    1, 2, ...) and the version first_version + i % versions."""
    i = np.arange(C)
    mask = (np.uint64(1) | ((i // versions).astype(np.uint64) << np.uint64(1))).astype(np.uint64)
    assert int(mask.max()) < (1 << NOBODYS_BIT)
    return mask, (first_version + i % versions).astype(np.int64)


def disjoint_classes(digests, versions):
    i = np.arange(digests * versions)
    return (np.uint64(1) << (i // versions).astype(np.uint64)).astype(np.uint64), (20 + i % versions).astype(np.int64)


def pool_by_class(cls_mask, cls_ver, cls_slots, seed, full_extra=2):
    """A registry in which class c offers exactly cls_slots[c] slots (0: its servants are full)."""
    rng = np.random.default_rng(11000 + seed)
    rows = []
    for c, want in enumerate(cls_slots):
        have = 0
        if want == 0:
            for _ in range(full_extra):
                nproc, load, mt, _ = _servant(rng, False)
                rows.append((c, nproc, 0, mt, min(mt, nproc), int(rng.random() < 0.3)))
        while have < want:
            ded = rng.random() < 0.3
            nproc, load, mt, run = _servant(rng, ded, roomy=want > 2000)
            n, _ = _slots(nproc, load, mt, run, ded)
            if n == 0:
                continue
            if have + n > want:
                run += have + n - want
                n = want - have
            rows.append((c, nproc, load, mt, run, int(ded)))
            have += n
    sv = _columns(rows, cls_mask, cls_ver, rng)
    assert len(class_table(sv)[1]) == len(cls_slots)
    return sv


def pool_by_tier(cls_mask, cls_ver, T0, M, seed, cls_weights=None, tier0_only=(), full=()):
    """A registry that offers exactly M slots, T0 of them in tier 0 (dedicated servants below half
    of their processors). tier0_only: classes whose servants are all dedicated and offer tier-0 slots
    only (their lists end where the tier does); full: classes without a free slot."""
    rng = np.random.default_rng(12000 + seed)
    C = len(cls_ver)
    w = np.ones(C) if cls_weights is None else np.asarray(cls_weights, float)
    w[list(full)] = 0
    user_w = w.copy()
    user_w[list(tier0_only)] = 0
    rows, t_have, m_have = [], 0, 0
    for c in full:
        nproc, load, mt, _ = _servant(rng, False)
        rows.append((c, nproc, 0, mt, min(mt, nproc), 0))
    seen = set(full)
    while t_have < T0:  # dedicated servants, until the tier is full
        c = int(rng.choice(C, p=w / w.sum()))
        tier1_room = (M - T0) - (m_have - t_have)
        pure = c in tier0_only or rng.random() < 0.5 or tier1_room < 64
        nproc, load, mt, run = _servant(rng, True, pure=pure)
        n, t = _slots(nproc, load, mt, run, True)
        if t == 0:
            continue
        if t_have + t > T0:
            cut = t_have + t - T0
            run, n, t = run + cut, n - cut, t - cut
        if n - t > tier1_room:
            continue
        rows.append((c, nproc, load, mt, run, 1))
        seen.add(c)
        t_have, m_have = t_have + t, m_have + n
    left = [c for c in range(C) if c not in seen and user_w[c] > 0]
    while m_have < M:  # everybody else: tier 1
        c = left.pop() if left else int(rng.choice(C, p=user_w / user_w.sum()))
        ded = rng.random() < 0.15
        nproc, load, mt, run = _servant(rng, ded)
        if ded:
            run = max(run, (nproc + 1) // 2)  # (at or above half: tier 1)
        n, t = _slots(nproc, load, mt, run, ded)
        if n == 0 or t:
            continue
        if m_have + n > M:
            run, n = run + m_have + n - M, M - m_have
        rows.append((c, nproc, load, mt, run, int(ded)))
        m_have += n
    for c in range(C):  # (a class nobody drew: one full servant keeps it in the table)
        if c not in {r[0] for r in rows}:
            nproc, load, mt, _ = _servant(rng, False)
            rows.append((c, nproc, 0, mt, min(mt, nproc), 0))
    sv = _columns(rows, cls_mask, cls_ver, rng)
    assert len(class_table(sv)[1]) == C
    return sv


def slot_counts(sv):
    """(T0, M) of a registry from the slot rules, without sorting anything."""
    ded = sv["priority"] == synth.PRIORITY_DEDICATED
    low = sv["memory_available"] < (10 << 30)
    m = t = 0
    for s in range(len(ded)):
        if low[s]:
            continue
        n, k = _slots(int(sv["num_processors"][s]), int(sv["current_load"][s]), int(sv["max_tasks"][s]),
                      int(sv["running_tasks"][s]), bool(ded[s]))
        m, t = m + n, t + k
    return t, m


# ---------------------------------------------------------------------------------------------
# Requests
# ---------------------------------------------------------------------------------------------
def requests(n, seed, digests=(0,), weights=None, unknown_frac=0.03, min_versions=(0, 20)):
    rng = np.random.default_rng(13000 + seed)
    d = np.asarray(digests)
    env = d[rng.choice(len(d), n, p=weights)]
    u = rng.random(n)
    env = np.where(u < unknown_frac / 2, UNKNOWN_ENV, np.where(u < unknown_frac, NOBODYS_BIT, env))
    minv = np.asarray(min_versions)[rng.integers(0, len(min_versions), n)]
    rip = FOREIGN + rng.integers(0, 1 << 16, n)
    return {"env_id": env.astype(np.uint32), "min_version": minv.astype(np.uint32), "requestor_ip": rip.astype(np.uint32)}


def eligibility(sv, tk):
    """[request, class] — task_class_mask: the class advertises the digest and its version is not
    below the request's minimum."""
    env, ver = class_table(sv)
    assert env.shape[1] == 1
    e = tk["env_id"].astype(np.int64)
    known = e < 64
    bit = (env[None, :, 0] >> np.where(known, e, 0).astype(np.uint64)[:, None]) & np.uint64(1)
    return (bit != 0) & known[:, None] & (ver[None, :].astype(np.int64) >= tk["min_version"].astype(np.int64)[:, None])


def consuming(sv, tk):
    return eligibility(sv, tk).any(axis=1)


def set_levels(sv, tk, cs, levels, digest=0):
    """Turns requests into unknown-digest ones or back so that exactly levels[k] consuming requests
    stand before chunk k (ascending k). Returns the new batch."""
    tk = {k: v.copy() for k, v in tk.items()}
    prev_k, prev_level = 0, 0
    for k in sorted(levels):
        lo, hi = prev_k * cs, k * cs
        con = consuming(sv, tk)
        have, want = int(con[:hi].sum()), levels[k]
        assert prev_level <= want <= prev_level + (hi - lo) and int(con[:lo].sum()) == prev_level, (k, want, have)
        idx = np.arange(lo, hi)
        if have > want:
            flip = idx[con[lo:hi]][::-1][:have - want]  # (the last of them: an unknown stretch at the chunk's end)
            tk["env_id"][flip] = UNKNOWN_ENV
        elif have < want:
            flip = idx[~con[lo:hi]][:want - have]
            tk["env_id"][flip] = digest
            tk["min_version"][flip] = 0
        assert int(consuming(sv, tk)[:hi].sum()) == want
        prev_k, prev_level = k, want
    return tk


def before_and_tail(con, cs, warm_len):
    """before[k]: consuming requests in front of chunk k (k = 0 .. K); tail[k]: those among the last
    warm_len requests of chunk k, for every chunk that is whole."""
    n = len(con)
    K = -(-n // cs)
    pre = np.concatenate([[0], np.cumsum(con)])
    before = np.array([pre[min(n, k * cs)] for k in range(K + 1)], np.int64)
    tail = np.array([pre[(k + 1) * cs] - pre[(k + 1) * cs - warm_len] if (k + 1) * cs <= n else 0 for k in range(K)],
                    np.int64)
    return before, tail


# ---------------------------------------------------------------------------------------------
# The global slot order, from the oracle; the walk of the tier's end, restated
# ---------------------------------------------------------------------------------------------
def global_order(sv):
    """Servant of every global rank: the oracle's answer to as many foreign requests for digest 0
    (which every servant of these pools advertises) as the registry could ever serve."""
    bound = int(np.minimum(sv["max_tasks"], sv["num_processors"]).astype(np.int64).sum()) + 1
    tk = {"env_id": np.zeros(bound, np.uint32), "min_version": np.zeros(bound, np.uint32),
          "requestor_ip": np.full(bound, FOREIGN, np.uint32)}
    got = O.dispatch(sv, tk, "sorted")[0]
    m = int((got < ENF).sum())
    assert (got[:m] < ENF).all() and (got[m:] == TIMEOUT).all()
    return got[:m].astype(np.int64)


def servant_classes(sv):
    """Class id of every servant (-1: takes no tasks), ids in order of first appearance."""
    env, ver = class_table(sv)
    sig = {(int(e[0]), int(v)): i for i, (e, v) in enumerate(zip(env, ver))}
    mask = np.asarray(sv["env_mask"]).reshape(len(sv["version"]), -1)
    return np.array([sig[(int(mask[s, 0]), int(sv["version"][s]))] if sv["max_tasks"][s] > 0 else -1
                     for s in range(len(mask))], np.int64)


def class_lists(sv):
    """(lists, T0, M): class c's list = the global ranks of its slots, ascending; T0 = the first rank
    of tier 1 (slot_tier: a dedicated servant's slot r with 2 r < num_processors is tier 0; the
    j-th slot a servant gives away is r = running_tasks + j)."""
    order = global_order(sv)
    M = len(order)
    seen = {}
    r = np.empty(M, np.int64)
    for p, s in enumerate(order):
        r[p] = int(sv["running_tasks"][s]) + seen.get(int(s), 0)
        seen[int(s)] = seen.get(int(s), 0) + 1
    tier0 = (sv["priority"][order] == synth.PRIORITY_DEDICATED) & (2 * r < sv["num_processors"][order].astype(np.int64))
    T0 = int(tier0.sum())
    assert tier0[:T0].all(), "tier 0 is a prefix of the order"
    cls = servant_classes(sv)[order]
    C = len(class_table(sv)[1])
    return [np.nonzero(cls == c)[0] for c in range(C)], T0, M


def level_cursors(lists, level):
    """The level guess: per class, its entries with a rank below `level`."""
    return np.array([int(np.searchsorted(l, level)) for l in lists], np.int64)


def zone_restate(sv, tk, cs, lead=ZONE_LEAD, trail=ZONE_TRAIL, warm_len=WARM_UP):
    """zone_walk, as zone_guess.h words it. Returns dict(T0, M, z_lo, z_hi, rows = z_hi - z_lo or 0,
    t_start, cursors = [rows, C] list positions (row 0: the level guess of t_start), level0)."""
    lists, T0, M = class_lists(sv)
    C = len(lists)
    el = eligibility(sv, tk)
    n = len(el)
    K = -(-n // cs)
    before, tail = before_and_tail(el.any(axis=1), cs, warm_len)
    out = dict(T0=T0, M=M, z_lo=0, z_hi=0, rows=0, t_start=0, cursors=np.zeros((0, C), np.int64), before=before,
               tail=tail)
    if M == 0 or K < 2 or C < 2 or T0 == 0 or T0 >= M:
        return out
    start = max(T0 - lead, 0)
    z_lo = next((k for k in range(1, K) if before[k] >= start), K)
    if z_lo >= K or before[z_lo] >= T0 + trail:  # the batch ends before the tier does, or starts behind it
        return out
    z_hi = z_lo + 1
    while z_hi < min(K, z_lo + ZONE_MAX_ROWS) and before[z_hi] - tail[z_hi - 1] < T0 + trail:
        z_hi += 1
    t_start = z_lo * cs - warm_len
    out.update(z_lo=z_lo, z_hi=z_hi, rows=z_hi - z_lo, t_start=t_start)
    if z_hi - z_lo < 2:
        return out  # (the header only: row 0 is chunk z_lo's own level guess)
    level = before[z_lo] - tail[z_lo - 1]
    x = level_cursors(lists, level)
    ends = np.array([len(l) for l in lists])
    rows = []
    for t in range(t_start, min(n, z_hi * cs)):
        if t == t_start + len(rows) * cs:  # chunk z_lo + len(rows) starts its replay here
            rows.append(x.copy())
            if len(rows) == z_hi - z_lo:
                break
        heads = np.array([lists[c][x[c]] if el[t, c] and x[c] < ends[c] else M for c in range(C)])
        c = int(heads.argmin())
        if heads[c] < M:
            x[c] += 1
    out.update(cursors=np.array(rows), level0=level)
    return out


def true_cursors(sv, tk, want, at):
    """Class cursors (list positions) in front of request `at`, from the oracle's placement: the
    slots a class has given away (without own-host requests a class is consumed from the front)."""
    cls = servant_classes(sv)
    C = len(class_table(sv)[1])
    w = want[:at]
    return np.bincount(cls[w[w < ENF].astype(np.int64)], minlength=C).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
class Case:
    """name, what it was made for, its switches (YDC_<KEY>), and (lazily) its pool and batch."""

    def __init__(self, name, path, build, switches, **promise):
        self.name, self.path, self._build, self.switches, self.promise = name, path, build, dict(switches), promise

    @functools.lru_cache(maxsize=None)
    def data(self):
        return self._build()

    @property
    def cs(self):
        return (int(self.switches["CHUNK_SIZE"]) + BLOCK - 1) // BLOCK * BLOCK  # (what the planner makes of it)

    def plan(self, n=None):
        sv, tk = self.data()
        kw = {k.lower(): int(v) for k, v in self.switches.items()}
        return guess_plan(sv, len(tk["env_id"]) if n is None else n, n_parts=self.promise.get("parts", 1), **kw)

    def __repr__(self):
        return self.name


def _spread(C, total, rng, small=()):
    """Slot counts per class: `small` first, the rest of `total` spread unevenly over the others."""
    rest = C - len(small)
    w = rng.random(rest) + 0.3
    big = np.maximum(1, (w / w.sum() * (total - sum(small))).astype(np.int64))
    return list(small) + [int(x) for x in big]


def _exact(name, form, C, n, cs, versions=1, slots=None, small=(), over=False, levels=None, seed=0, own_frac=0.0,
           cut=None, unknown_frac=0.03, **switches):
    """An exact pool of C classes. slots: per class (else spread: 1.3 n, or 0.55 n when the pool is
    oversubscribed); levels: {chunk: consuming requests before it} or a function of (M, cs, n)."""
    sw = dict(CHUNK_SIZE=cs, **switches)

    def build():
        rng = np.random.default_rng(14000 + seed)
        mask, ver = classes_with_digest0(C, versions)
        per = slots if slots is not None else _spread(C, int((0.55 if over else 1.3) * n), rng, small)
        sv = pool_by_class(mask, ver, per, seed)
        tk = requests(n, seed, unknown_frac=unknown_frac)
        if own_frac:
            # The control: a tenth of the requests — the last of every chunk among them — come from the
            # host of the very servant they would have been placed on: they step over its slots, and a
            # chunk that ends there hands a state with holes to its successor, which no level guess has.
            got = O.dispatch(sv, tk, "sorted")[0]
            own = rng.random(n) < own_frac
            own[cs - 1::cs] = True
            own &= got < ENF
            tk["requestor_ip"] = np.where(own, sv["ip"][np.where(own, got, 0)], tk["requestor_ip"]).astype(np.uint32)
        lv = levels(sum(per), cs, n) if callable(levels) else levels
        if lv:
            tk = set_levels(sv, tk, cs, lv)
        return sv, tk

    return Case(name, form, build, sw, C=C, over=over, exact=own_frac == 0, cut=cut, slots=slots,
                levels=levels is not None)


def _edge_levels(M, cs, n):
    """Levels on a multiple of 64, on n_slots - 1 and on n_slots (an oversubscribed pool: the chunk
    between them holds one consuming request), the rest of the batch beyond."""
    k = 5 + -(-(M - 257) // cs) + 1  # (room behind chunk 5 for the M - 257 consuming requests still to come)
    assert (k + 2) * cs <= n, (M, cs, n)
    return {2: 64, 5: 256, k: M - 1, k + 1: M}


def _tile_levels(M, cs, n):
    """Levels on both sides of multiples of the tile table's 512 slots, and (oversubscribed) in the
    last tile and past n_slots."""
    k1, k2 = 512 // cs + 1, 1024 // cs + 2
    k3 = (M + 2 * cs) // cs + 2
    assert (k3 + 1) * cs <= n and 1024 < M - 3
    return {k1: 511, k2: 1024, k3 - 1: M - 3, k3: M}


@functools.lru_cache(maxsize=None)
def exact_cases():
    big = 4097
    out = [
        # ---- F1: bin sort and level table
        _exact("F1-C1-fill", TABLE_FILL, 1, 4096, 64, seed=1),
        _exact("F1-C3-fill-short-and-full", TABLE_FILL, 3, 4096, 64, slots=[5200, 40, 0], seed=2,
               levels={3: 128, 9: 512, 20: 1216}),
        _exact("F1-C4-fill-edges", TABLE_FILL, 4, 8192, 128, over=True, levels=_edge_levels, seed=3),
        _exact("F1-C4-rings-of-32", TABLE, 4, 4096, 64, seed=4, RING_TOTAL=256),
        _exact("F1-C5", TABLE, 5, 4096, 64, small=(33,), seed=5, levels={4: 192, 11: 640}),
        _exact("F1-C8-edges", TABLE, 8, 16384, 256, over=True, small=(63, 0), levels=_edge_levels, seed=6),
        _exact("F1-C8-chunks-of-512", TABLE, 8, 16384, 512, seed=7),
        # ---- F2: the wave-cooperative search (radix path)
        _exact("F2-lists-1-63-64-65", WAVE, 4, 4096, 64, slots=[1, 63, 64, 65], seed=8, BINSORT=0),
        _exact("F2-list-4097", WAVE, 2, 8192, 128, slots=[big, 2900], seed=9, BINSORT=0),
        _exact("F2-C3-4097-and-64", WAVE, 3, 8192, 128, slots=[64, big, 3000], seed=10, BINSORT=0),
        # ---- F3: the quartile search
        _exact("F3-bins-C9-ranges-1-5", QUARTILE, 9, 4096, 64, small=(1, 2, 3, 4, 5), seed=11),
        _exact("F3-bins-C64", QUARTILE, 64, 8192, 128, seed=12, small=(1, 0, 2)),
        _exact("F3-tiles-C9", QUARTILE_TILES, 9, 8192, 64, over=True, levels=_tile_levels, seed=13, BINSORT=0),
        _exact("F3-tiles-C17", QUARTILE_TILES, 17, 8192, 128, over=True, levels=_tile_levels, small=(1, 2, 3),
               seed=14, BINSORT=0),
        _exact("F3-tiles-C64", QUARTILE_TILES, 64, 16384, 256, over=True, levels=_tile_levels, small=(4, 5, 0),
               seed=15, BINSORT=0),
        # ---- F4: one class, no list of ranks
        _exact("F4-one-class", ONE, 1, 4096, 64, seed=16, BINSORT=0),
        _exact("F4-one-class-over", ONE, 1, 8192, 128, over=True, levels=_edge_levels, seed=17, BINSORT=0),
        # ---- F5: k_guess_init
        _exact("F5-C16-no-own-guess", INIT, 16, 4096, 64, seed=18, OWN_GUESS=0),
        _exact("F5-C100-two-words", INIT, 100, 8192, 128, versions=3, seed=19),
        _exact("F5-C200-four-words", INIT, 200, 8192, 128, versions=3, seed=20, small=(0, 1)),
        # ---- F7: the warm-up
        _exact("F7-chunks-256", TABLE, 6, 16384, 256, seed=21),
        _exact("F7-warm-1", TABLE_FILL, 2, 4096, 64, seed=22, WARM_UP=1),
        _exact("F7-warm-17", QUARTILE, 12, 4096, 64, seed=23, WARM_UP=17),
        _exact("F7-warm-64-is-the-whole-chunk", TABLE, 7, 4096, 64, seed=24, WARM_UP=64),
        _exact("F7-unknown-stretch-tail-0", QUARTILE_TILES, 10, 8192, 128, seed=25, BINSORT=0,
               levels={3: 3 * 128 - 70, 7: 7 * 128 - 70 - 128}),
        _exact("F7-last-chunk-of-one", TABLE, 5, 4097, 64, seed=26),
        _exact("F7-two-batches", QUARTILE, 20, 8192, 64, seed=27, cut=4096 + 29),
        _exact("F7-two-batches-tiles", QUARTILE_TILES, 20, 8192, 64, seed=28, cut=4096 + 29, BINSORT=0),
    ]
    return tuple(out)


def _disjoint(name, digests, versions, n, cs, seed, **switches):
    """Disjoint digests: `digests` parts of `versions` classes each; part 0 is exhausted a third of
    the way through the batch while the others are not."""
    C = digests * versions

    def build():
        rng = np.random.default_rng(15000 + seed)
        mask, ver = disjoint_classes(digests, versions)
        share = n // digests
        per = []
        for d in range(digests):
            tot = share // 3 if d == 0 else int(1.4 * share)
            per += _spread(versions, tot, rng)
        sv = pool_by_class(mask, ver, per, seed)
        return sv, requests(n, seed, digests=np.arange(digests))

    return Case(name, QUARTILE, build, dict(CHUNK_SIZE=cs, **switches), C=C, exact=True, parts=digests, cut=None,
                over=True, levels=False, slots=None)


@functools.lru_cache(maxsize=None)
def disjoint_cases():
    return (_disjoint("F6-4x3", 4, 3, 8192, 64, 30), _disjoint("F6-8x5", 8, 5, 8192, 128, 31))


@functools.lru_cache(maxsize=None)
def control_cases():
    """One pool per form with a tenth of the requests from servants' own hosts: not exact, the
    replay counter must move."""
    return (
        _exact("control-table-fill", TABLE_FILL, 3, 4096, 64, seed=40, own_frac=0.1),
        _exact("control-table", TABLE, 8, 4096, 64, seed=41, own_frac=0.1),
        _exact("control-wave", WAVE, 3, 4096, 64, seed=42, own_frac=0.1, BINSORT=0),
        _exact("control-quartile", QUARTILE, 12, 4096, 64, seed=43, own_frac=0.1),
        _exact("control-quartile-tiles", QUARTILE_TILES, 12, 4096, 64, seed=44, own_frac=0.1, BINSORT=0),
        _exact("control-one", ONE, 1, 4096, 64, seed=45, own_frac=0.1, BINSORT=0),
        _exact("control-init", INIT, 16, 4096, 64, seed=46, own_frac=0.1, OWN_GUESS=0),
    )


# ---- the walk of the tier's end -------------------------------------------------------------
def _walk(name, C, T0, M, n, cs, lead=None, trail=None, versions=2, seed=0, digests=4, levels=None, first=0,
          tier0_only=(), full=(), solo=None, unknown_block=None, walk=True, cls_weights=None, rough=None,
          **switches):
    """A walk pool: C classes (digest 0 + the bits of the class number over `digests` others; versions
    19 .. : a request with min_version 20 is not eligible for the lowest), exactly M slots, T0 of them
    in tier 0. solo = (class, at, count): `count` requests in a row from `at` on for a digest that only
    that class advertises; unknown_block = at: 64 unknown-digest requests from there; first: requests
    committed as a batch of their own before the one under test; rough = at: up to there every known
    request is eligible for every class (the level guess is exact), behind it most requests ask for
    one of the other digests, half of them at min_version 20 (the true cursors leave the level by
    dozens of list positions, and the walk has to follow them)."""
    sw = dict(CHUNK_SIZE=cs, ZONE_GUESS=2, BINSORT=0, **switches)
    if lead is not None:
        sw["ZONE_LEAD"] = lead
    if trail is not None:
        sw["ZONE_TRAIL"] = trail
    solo_bit = 40

    def build():
        mask, ver = classes_with_digest0(C, versions, first_version=19 if versions > 1 else 20)
        if solo:
            mask = mask.copy()
            mask[solo[0]] |= np.uint64(1) << np.uint64(solo_bit)
        sv = pool_by_tier(mask, ver, T0, M, seed, cls_weights=cls_weights, tier0_only=tier0_only, full=full)
        nd = max(1, _bits(-(-C // versions)))
        # (most requests ask for digest 0: inside a tier the true cursors then stay within a few list
        # positions of the level, and a walk started from the level guess is on the true track within
        # a chunk — the condition tests/test_guess_edges_model.py asserts row by row)
        tk = requests(n, seed, digests=np.arange(nd + 1), weights=[0.85] + [0.15 / nd] * nd, unknown_frac=0.02,
                      min_versions=(0, 0, 0, 0, 0, 20))
        if rough is not None:
            wild = requests(n, seed + 500, digests=np.arange(nd + 1), weights=[0.3] + [0.7 / nd] * nd, unknown_frac=0.02)
            known = tk["env_id"] < NOBODYS_BIT
            tk["env_id"][:rough] = np.where(known[:rough], 0, tk["env_id"][:rough])
            tk["min_version"][:rough] = 0
            for k in ("env_id", "min_version"):
                tk[k][rough:] = wild[k][rough:]
        if solo:
            tk["env_id"][solo[1]:solo[1] + solo[2]] = solo_bit
            tk["min_version"][solo[1]:solo[1] + solo[2]] = 0
        if unknown_block is not None:
            tk["env_id"][unknown_block:unknown_block + 64] = UNKNOWN_ENV
        if levels:
            tk = set_levels(sv, tk, cs, levels)
        return sv, tk

    return Case(name, "walk" if walk else "no walk", build, sw, C=C, T0=T0, M=M, first=first,
                lead=ZONE_LEAD if lead is None else lead, trail=ZONE_TRAIL if trail is None else trail)


@functools.lru_cache(maxsize=None)
def walk_cases():
    M = 4096
    return (
        # ---- where the zone falls
        _walk("W-T0-0", 9, 0, M, 4096, 64, 512, 256, seed=50),
        _walk("W-T0-M", 9, M, M, 4096, 64, 512, 256, seed=51),
        _walk("W-T0-1", 16, 1, M, 4096, 64, 512, 256, seed=52),
        _walk("W-T0-63", 9, 63, M, 4096, 64, 512, 256, seed=53),
        _walk("W-T0-64", 17, 64, M, 4096, 64, 512, 256, seed=54),
        _walk("W-T0-65", 32, 65, M, 4096, 64, 512, 256, seed=55),
        _walk("W-T0-M-1", 16, M - 1, M, 8192, 64, 512, 256, seed=56),
        _walk("W-batch-ends-before", 9, 6000, 8000, 4096, 64, 512, 256, seed=57),
        _walk("W-batch-starts-behind", 9, 1, M, 4096, 64, 512, 16, seed=58),
        _walk("W-second-batch", 16, 2500, 6000, 8192, 64, 512, 256, seed=59, first=1000 + 29),
        _walk("W-second-batch-behind", 16, 900, 6000, 8192, 64, 512, 256, seed=60, first=1024),
        _walk("W-header-only", 9, 1000, M, 4096, 64, 16, 16, seed=61, levels={16: 1000}),
        _walk("W-cap-32-default-lead", 16, 3000, 6000, 8192, 64, seed=62),
        _walk("W-reaches-last-chunk", 17, 4000, 6000, 4096 + 64 + 37, 64, 512, 1024, seed=63),
        # ---- the rings
        _walk("W-C9", 9, 1500, M, 4096, 64, 512, 256, seed=64),
        _walk("W-C9-rough", 9, 1500, M, 4096, 64, 512, 256, seed=77, rough=1100),
        _walk("W-C17-rough-default-lead", 17, 3000, 6000, 8192, 64, seed=78, rough=800),
        _walk("W-C32-rough-chunks-128", 32, 3000, 7000, 8192, 128, 512, 256, versions=3, seed=79, rough=2700),
        _walk("W-C16-chunks-128", 16, 3000, 7000, 8192, 128, 512, 256, seed=65),
        _walk("W-C17", 17, 1500, M, 4096, 64, 512, 256, seed=66),
        _walk("W-C32-chunks-128", 32, 3000, 7000, 8192, 128, 512, 256, versions=3, seed=67),
        _walk("W-C33-refused", 33, 1500, M, 4096, 64, 512, 256, versions=3, seed=68, walk=False),
        _walk("W-C64-rings-4096", 64, 1500, M, 4096, 64, 512, 256, versions=3, seed=69, RING_TOTAL=4096),
        _walk("W-one-class-200-in-a-row", 12, 1500, 5000, 4096, 64, 512, 256, seed=70, solo=(3, 1400, 200),
              cls_weights=[1, 1, 1, 12] + [1] * 8),
        _walk("W-lists-end-and-empty", 12, 1500, M, 4096, 64, 512, 256, seed=71, tier0_only=(2, 5), full=(7,)),
        _walk("W-all-exhausted", 10, 1500, 1800, 4096, 64, 512, 1024, seed=72),
        _walk("W-unknown-block", 10, 1500, M, 4096, 64, 512, 256, seed=73, unknown_block=1472),
        # ---- lead and trail
        _walk("W-lead-128", 16, 1500, M, 4096, 64, 128, 256, seed=74),
        _walk("W-lead-128-chunks-128", 20, 3000, 7000, 8192, 128, 128, 256, seed=75),
        # ---- a chunk size that is no multiple of 64: rounded up to 128
        _walk("W-chunks-96", 16, 3000, 7000, 8192, 96, 512, 256, seed=76),
    )


def all_cases():
    return exact_cases() + disjoint_cases() + control_cases() + walk_cases()


def case(name):
    return {c.name: c for c in all_cases()}[name]


def stages(case):
    """The batches of a case in the order they are committed, each with the registry it meets:
    [(servants, requests)] — two where the case cuts its batch (`cut`: both halves are under test;
    `first`: the requests in front only prepare the registry)."""
    sv, tk = case.data()
    cut = case.promise.get("cut") or case.promise.get("first") or 0
    if not cut:
        return [(sv, tk)]
    head = {k: v[:cut] for k, v in tk.items()}
    run = O.dispatch(sv, head, "sorted")[2]
    return [(sv, head), (dict(sv, running_tasks=run), {k: v[cut:] for k, v in tk.items()})]
