"""Pools made for the host-alias paths (ydc_set_host_aliases), shared by tests/test_alias_model.py
(CPU) and tests/test_alias_gpu.py.

A case is servants given by their LOCATION strings and requests given by their requestor ADDRESS
strings; tests/alias_reference.py interns them into the device API's form: one primary host id per
servant (the `ip` column), further (host id, servant row) alias pairs, one id per request.

Every case (but those of ONE_SERVANT, see there) is built so that the aliases DECIDE placements:
the reference's answers with the alias pairs stripped differ from its answers with them in at
least 5 % of the requests (`single` and `duplicates`: in at least one). DIFFER holds the number of
differing requests per case; tests/test_alias_model.py asserts it. A case in which the aliases
decide nothing proves nothing.
"""
import functools

import numpy as np

from tests import alias_reference as A
from yadcc_amd import synth

GIB = 1 << 30
UNKNOWN_ENV = 0xFFFF
COLS = ("version", "num_processors", "current_load", "max_tasks", "running_tasks", "priority",
        "total_memory", "memory_available", "env_mask", "ip", "port")


def sv(rows):
    """Raw servant columns from dicts over the defaults of tests/cases.py's handmade cases."""
    d = {c: [] for c in COLS}
    for r in rows:
        base = dict(version=20, num_processors=16, current_load=0, max_tasks=8, running_tasks=0,
                    priority=2, total_memory=64 * GIB, memory_available=32 * GIB, env_mask=1, ip=0,
                    port=8335)
        base.update(r)
        for c in COLS:
            d[c].append(base[c])
    u64 = ("total_memory", "memory_available", "env_mask")
    return {c: np.array(v, dtype=np.uint64 if c in u64 else np.uint32) for c, v in d.items()}


class Case:
    """name; locations (per servant); sv (raw columns, `ip` = the primary host id); requestors (per
    request); tk (env_id, min_version, requestor_ip = the requestor's id); aliases = (host id,
    servant row) columns; floor: the least number of requests the aliases must decide."""

    def __init__(self, name, locations, columns, requestors, env_id, min_version, floor=0.05,
                 more_aliases=()):
        assert len(set(locations)) == len(locations), "a location twice is one servant"
        self.name, self.locations, self.requestors = name, list(locations), list(requestors)
        primary, (aip, asv), rid, self.names = A.intern(self.locations, self.requestors)
        self.sv = {k: np.array(v, copy=True) for k, v in columns.items()}
        self.sv["ip"] = primary
        self.n_servants, self.n_requests = len(self.locations), len(self.requestors)
        for ip, s in more_aliases:  # (given by address string)
            aip = np.append(aip, np.uint32(self.names[ip]))
            asv = np.append(asv, np.uint32(s))
        self.aliases = (aip.astype(np.uint32), asv.astype(np.uint32))
        self.tk = {"env_id": np.asarray(env_id, np.uint32), "min_version": np.asarray(min_version, np.uint32),
                   "requestor_ip": rid}
        assert len(self.tk["env_id"]) == len(self.tk["min_version"]) == self.n_requests
        self.floor = max(1, int(np.ceil(floor * self.n_requests))) if isinstance(floor, float) else floor

    def __repr__(self):
        return "<alias case %s: %d servants, %d requests, %d alias pairs>" % (
            self.name, self.n_servants, self.n_requests, len(self.aliases[0]))

    def slice(self, lo, hi):
        """Requests lo .. hi as (requestor strings, task columns)."""
        return self.requestors[lo:hi], {k: v[lo:hi] for k, v in self.tk.items()}


def personalities(n, n_requests, n_envs, seed, oversubscribed=False, initial_running=False):
    """n random servants (yadcc_amd.synth) whose slots are about 1.25 (oversubscribed: 0.5) of the
    requests."""
    cols = synth.make_servants(n, n_tasks_hint=max(n_requests, 2 * n), n_envs=n_envs, seed=seed,
                               oversubscribed=oversubscribed)
    if initial_running:
        rng = np.random.default_rng(seed + 7)
        top = np.minimum(cols["max_tasks"], cols["num_processors"]).astype(np.int64)
        cols["running_tasks"] = (rng.random(n) * (top + 3)).astype(np.uint32)
    return cols


def _requests(rng, n, requestors, weights, n_envs, unknown=0.0, min_version_20=0.5):
    w = np.asarray(weights, np.float64)
    who = rng.choice(len(requestors), size=n, p=w / w.sum())
    env = rng.integers(0, n_envs, n)
    if unknown:
        env = np.where(rng.random(n) < unknown, UNKNOWN_ENV, env)
    minv = np.where(rng.random(n) < min_version_20, 20, 0)
    return [requestors[i] for i in who], env, minv


# ---------------------------------------------------------------------------------------------
# The made cases
# ---------------------------------------------------------------------------------------------
def bracket():
    """40 servants at bracketed IPv6 locations, ten hosts with two servants; requests from the hosts,
    from the short forms "[:" and "[" every bracketed servant answers to, and from near misses."""
    locs = ["[::%d]:8335" % k for k in range(1, 31)] + ["[::%d]:9000" % k for k in range(1, 11)]
    cols = personalities(40, 400, 2, seed=101)
    # (the first of the registry — `self` for "[" and "[:" while it is free — are the best choice)
    for k, v in dict(priority=1, num_processors=64, max_tasks=60, current_load=0, version=20, env_mask=3,
                     memory_available=64 * GIB).items():
        cols[k][:3] = v
    rng = np.random.default_rng(102)
    hosts = ["[::%d]" % k for k in range(1, 31)]
    misses = ["::%d" % k for k in (1, 7, 30)] + ["[::%d" % k for k in (1, 7, 30)] + ["[::1]:8335", "[::7]:9000", ""]
    who = hosts + ["[:", "["] + misses
    req, env, minv = _requests(rng, 400, who, [0.4 / 30] * 30 + [0.15, 0.15] + [0.3 / len(misses)] * len(misses), 2)
    return Case("bracket", locs, cols, req, env, minv)


def everybody():
    """300 servants of one or two slots that all answer to "[": a third of the requests come from
    there, so `self` moves down the registry as servants fill. More requests than slots: the
    fall-back to `self` and Timeout both occur (asserted by the model test)."""
    S, N = 300, 660
    rng = np.random.default_rng(111)
    rows = [dict(num_processors=8, current_load=int(rng.integers(0, 3)), max_tasks=int(rng.integers(1, 3)),
                 version=20 if rng.random() < 0.8 else 19, priority=1 if rng.random() < 0.2 else 2)
            for _ in range(S)]
    locs = ["[::%x]:8335" % (k + 1) for k in range(S)]
    who = ["[", "[::%x]" % int(rng.integers(1, S + 1)), "172.16.0.9", "::2"]
    req, env, minv = _requests(rng, N, who, [1, 0.3, 1, 0.7], 1, min_version_20=0.3)
    req[400:500] = ["["] * 100  # (the slots run out inside this run: the last free servant is `self`)
    return Case("everybody", locs, sv(rows), req, env, minv)


def chain():
    """Nested addresses in four classes. "a:b:1" takes no tasks and "a:c:2" lacks digest 0: neither
    may ever be `self` for such a request. The alias id "a" of "a:b:1", "a:c:2" and "a:b:7" IS the
    primary id of "a:9"."""
    locs = ["a:b:1", "a:c:2", "a:9", "a:b:7"]
    cols = sv([dict(max_tasks=0, env_mask=0b11, version=20),
               dict(max_tasks=6, env_mask=0b10, version=21),
               dict(max_tasks=6, env_mask=0b11, version=20, current_load=2),
               dict(max_tasks=6, env_mask=0b01, version=19, current_load=1)])
    rng = np.random.default_rng(121)
    req, env, minv = _requests(rng, 40, ["a", "a:b", "a:c", "a:", "a:b:1"], [3, 2, 2, 1, 1], 2, min_version_20=0.0)
    return Case("chain", locs, cols, req, env, minv)


def single():
    """A class of ONE servant (HostTables::cls_single) that its requestor reaches only through an
    alias, next to a class of eight. It is idle and dedicated: without the alias it takes the
    requests of its own host."""
    locs = ["x:y:1"] + ["10.0.0.%d:8335" % k for k in range(1, 9)]
    cols = sv([dict(version=21, priority=1, max_tasks=12, num_processors=32)] +
              [dict(max_tasks=3, current_load=k % 3) for k in range(8)])
    req = ["x"] * 6 + ["x:y"] * 3 + ["10.0.0.1"] * 3 + ["x"] * 20
    return Case("single", locs, cols, req, [0] * len(req), [0] * len(req), floor=1)


def dedicated():
    """`self`, reached through an alias, is the dedicated servant that owns the globally best slots
    (the shape of burst_from_best in tests/cases.py)."""
    locs = ["[::1]:8335", "10.0.0.2:8335", "10.0.0.3:8335"]
    cols = sv([dict(priority=1, max_tasks=15, num_processors=32), dict(max_tasks=6), dict(max_tasks=6)])
    req = ["["] * 12 + ["172.16.0.9"] * 3 + ["[:"] * 14
    return Case("dedicated", locs, cols, req, [0] * len(req), [0] * len(req))


def huge():
    """Two aliased servants with capacities of 2^21 and more: the fp64 sort key (huge_capacity in
    tests/cases.py)."""
    locs = ["h:a:1", "h:b:2"]
    cols = sv([dict(num_processors=3_000_000, max_tasks=3_000_000, running_tasks=2_999_990),
               dict(num_processors=5_000_011, max_tasks=5_000_000, running_tasks=4_999_985,
                    current_load=4_999_000, priority=1)])
    req = (["h"] * 4 + ["h:a"] * 3 + ["172.16.0.9"] * 2 + ["h:b"] * 3 + ["h"] * 3) * 2
    return Case("huge", locs, cols, req, [0] * len(req), [0] * len(req))


def many_classes():
    """150 digests, a handful per servant, about one class per servant (the shape of wide_envs_150
    in tests/cases.py): the matching kernels for more than 256 classes. Bracketed locations, a
    tenth of the requests from "["."""
    S, N = 640, 2000
    cols = personalities(S, N, 150, seed=12)
    rng = np.random.default_rng(131)
    locs = ["[::%x]:8335" % (k + 1) for k in range(S)]
    who = ["[", "[:", "172.16.0.9"] + ["[::%x]" % (k + 1) for k in range(0, S, 7)]
    rest = len(who) - 3
    req, env, minv = _requests(rng, N, who, [0.1, 0.05, 0.55] + [0.3 / rest] * rest, 150, unknown=0.01)
    return Case("many_classes", locs, cols, req, env, minv)


def duplicates():
    """The alias list names a pair twice, and names a pair that is a servant's primary pair."""
    locs = ["p:q:%d" % k for k in range(1, 4)] + ["p:r:%d" % k for k in range(1, 4)]
    cols = sv([dict(max_tasks=3, current_load=k % 2) for k in range(6)])
    req = (["p"] * 3 + ["p:q"] * 2 + ["p:r"] * 2 + ["172.16.0.9"]) * 3
    return Case("duplicates", locs, cols, req, [0] * len(req), [0] * len(req), floor=1,
                more_aliases=[("p", 4), ("p", 4), ("p", 0), ("p:q", 1), ("p:r", 5)])


MADE = (bracket, everybody, chain, single, dedicated, huge, many_classes, duplicates)


# ---------------------------------------------------------------------------------------------
# Random cases
# ---------------------------------------------------------------------------------------------
def random_locations(rng, n):
    """n distinct locations of 1 to 4 ':'-separated parts, a part being one or two letters of
    "abc" (rarely empty): prefixes collide often."""
    out, seen = [], set()
    while len(out) < n:
        parts = []
        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.choice([0, 1, 1, 1, 2, 2, 2, 2]))
            parts.append("".join("abc"[int(x)] for x in rng.integers(0, 3, k)))
        loc = ":".join(parts)
        if loc not in seen:
            seen.add(loc)
            out.append(loc)
    return out


def random_case(seed, n_servants, n_requests):
    """Locations from random_locations; requestors drawn from EVERY prefix of every location,
    matching or not (the construction of td_scenarios.address_prefix_forms); 1 to 8 digests; with
    and without oversubscription and initial running_tasks."""
    rng = np.random.default_rng(seed)
    n_envs = int(rng.integers(1, 9))
    oversubscribed, initial_running = bool(rng.integers(2)), bool(rng.integers(2))
    cols = personalities(n_servants, n_requests, n_envs, seed, oversubscribed, initial_running)
    locs = random_locations(rng, n_servants)
    prefixes = sorted({loc[:i] for loc in locs for i in range(len(loc) + 1)})
    req, env, minv = _requests(rng, n_requests, prefixes, np.ones(len(prefixes)), n_envs, unknown=0.02)
    return Case("random-%d-S%d-N%d" % (seed, n_servants, n_requests), locs, cols, req, env, minv)


# (seed, servants, requests): 60 cases over servants in {3, 40, 300} x requests in {1, 63, 64, 65,
# 700, 5000}, three or four per shape (300 x 5000: one). Per shape the seeds were tried in ascending
# order; a seed whose case misses the 5 % condition was replaced by the next one and is not counted.
RANDOM_SPECS = (
    (1022, 3, 1), (1046, 3, 1), (1083, 3, 1), (1146, 3, 1), (1166, 3, 63),
    (1169, 3, 63), (1176, 3, 63), (1177, 3, 63), (1181, 3, 64), (1186, 3, 64),
    (1192, 3, 64), (1203, 3, 64), (1205, 3, 65), (1206, 3, 65), (1208, 3, 65),
    (1215, 3, 65), (1216, 3, 700), (1221, 3, 700), (1222, 3, 700), (1223, 3, 5000),
    (1240, 3, 5000), (1242, 3, 5000), (1341, 40, 1), (1423, 40, 1), (1522, 40, 1),
    (2121, 40, 1), (2135, 40, 63), (2164, 40, 63), (2187, 40, 63), (20013, 40, 63),
    (2240, 40, 64), (2254, 40, 64), (2266, 40, 64), (20029, 40, 64), (2341, 40, 65),
    (2357, 40, 65), (2359, 40, 65), (2413, 40, 700), (2438, 40, 700), (2444, 40, 700),
    (2445, 40, 5000), (2448, 40, 5000), (2451, 40, 5000), (4374, 300, 1), (4941, 300, 1),
    (5703, 300, 1), (6710, 300, 1), (6841, 300, 63), (6895, 300, 63), (6924, 300, 63),
    (7004, 300, 64), (7017, 300, 64), (7052, 300, 64), (7075, 300, 65), (7372, 300, 65),
    (7410, 300, 65), (7781, 300, 700), (8453, 300, 700), (9221, 300, 700), (10140, 300, 5000),
)
SHAPES = [(S, N) for S in (3, 40, 300) for N in (1, 63, 64, 65, 700, 5000)]

# With ONE servant no answer can depend on who `self` is (the only candidate is granted whether it
# is `self` or not), so these shapes cannot meet the condition; they run for the interning, the
# table of one entry and the fall-back, and are compared with the reference like the others.
ONE_SERVANT_SPECS = tuple((900 + i, 1, N) for i, N in enumerate((1, 63, 64, 65, 700, 5000)))


def verbatim(locations, columns, requestors, tk, running=None):
    """The verbatim reference class (oracle/refbind.py: RefDispatcher) on the strings: one
    keep_servant_alive per servant with its location, then one wait_for_starting_new_task per
    request with the requestor's address, in order. Initial running_tasks are primed by grants on a
    private digest before the real personality is installed (a heartbeat replaces the personality
    and keeps running_tasks, task_dispatcher.cc:195-201).
    -> (servant index or IDX_* per request, running_tasks afterwards)."""
    from oracle import refbind as R
    ref = R.RefDispatcher()
    running = columns["running_tasks"] if running is None else running
    em = columns["env_mask"]
    for s, loc in enumerate(locations):
        r = int(running[s])
        if r:
            ref.keep_servant_alive(loc, ["prime"], r, r, 0, memory_available=64 * GIB)
            for _ in range(r):
                assert ref.wait_for_starting_new_task("nobody", "prime")[2] == loc
        words = [int(em[s])] if em.ndim == 1 else [int(w) for w in em[s]]
        envs = ["d%d" % (64 * k + b) for k, w in enumerate(words) for b in range(64) if w >> b & 1]
        ref.keep_servant_alive(loc, envs, int(columns["max_tasks"][s]), int(columns["num_processors"][s]),
                               int(columns["current_load"][s]), priority=int(columns["priority"][s]),
                               version=int(columns["version"][s]), total_memory=int(columns["total_memory"][s]),
                               memory_available=int(columns["memory_available"][s]))
    row_of = {loc: s for s, loc in enumerate(locations)}
    out = np.empty(len(requestors), np.uint32)
    for t, requestor in enumerate(requestors):
        st, _, loc = ref.wait_for_starting_new_task(requestor, "d%d" % int(tk["env_id"][t]),
                                                    min_version=int(tk["min_version"][t]))
        out[t] = row_of[loc] if st == R.OK else A.IDX_ENV_NOT_FOUND if st == R.ENV_NOT_FOUND else A.IDX_TIMEOUT
    after = np.zeros(len(locations), np.uint32)
    for item in ref.dump_internals().get("servants", []):
        after[row_of[item["location"]]] = item["running_tasks"]
    ref.close()
    return out, after


PURE_PYTHON_LIMIT = 200_000  # requests x servants up to which tests/alias_reference.py is the reference


@functools.lru_cache(maxsize=None)
def want(case):
    """The reference's answers for the whole case, computed once: (servant_idx, utilisation,
    running_tasks after). Beyond PURE_PYTHON_LIMIT the verbatim reference class gives the placement
    where it is built (the doubles then follow from the placement: see utilisations)."""
    from oracle import refbind as R
    if case.n_requests * case.n_servants <= PURE_PYTHON_LIMIT or not R.available():
        return A.dispatch(case.locations, case.sv, case.requestors, case.tk)
    idx, run = verbatim(case.locations, case.sv, case.requestors, case.tk)
    return idx, utilisations(case.sv, idx), run


def utilisations(columns, idx, running=None):
    """The double the reference computed when it made each of the grants `idx` (task_dispatcher.cc:
    440-441: running_tasks / GetCapacityAvailable at that moment); -1.0 where nothing was granted."""
    run = [int(x) for x in (columns["running_tasks"] if running is None else running)]
    out = np.full(len(idx), -1.0, np.float64)
    for t, s in enumerate(idx):
        s = int(s)
        if s >= A.IDX_ENV_NOT_FOUND:
            continue
        cap = A.capacity_available(int(columns["num_processors"][s]), int(columns["current_load"][s]),
                                   int(columns["max_tasks"][s]), int(columns["total_memory"][s]),
                                   int(columns["memory_available"][s]), run[s], A.MIN_MEMORY_DEFAULT)
        out[t] = float(run[s]) / cap
        run[s] += 1
    return out


def differing(case):
    """Number of requests the reference answers differently once the alias pairs are stripped
    (the comparison reduced to the primary address)."""
    with_aliases = A.dispatch(case.locations, case.sv, case.requestors, case.tk)[0]
    without = A.dispatch(case.locations, case.sv, case.requestors, case.tk, same_host=A.is_primary_address)[0]
    return int((with_aliases != without).sum())


# Requests the aliases decide, per case (asserted by tests/test_alias_model.py).
DIFFER = {
    "bracket": 33, "everybody": 96, "chain": 9, "single": 29,
    "dedicated": 24, "huge": 6, "many_classes": 274, "duplicates": 8,
    "random-1022-S3-N1": 1, "random-1046-S3-N1": 1, "random-1083-S3-N1": 1, "random-1146-S3-N1": 1,
    "random-1166-S3-N63": 7, "random-1169-S3-N63": 7, "random-1176-S3-N63": 20, "random-1177-S3-N63": 6,
    "random-1181-S3-N64": 5, "random-1186-S3-N64": 7, "random-1192-S3-N64": 6, "random-1203-S3-N64": 13,
    "random-1205-S3-N65": 6, "random-1206-S3-N65": 6, "random-1208-S3-N65": 4, "random-1215-S3-N65": 13,
    "random-1216-S3-N700": 35, "random-1221-S3-N700": 40, "random-1222-S3-N700": 44, "random-1223-S3-N5000": 269,
    "random-1240-S3-N5000": 530, "random-1242-S3-N5000": 433, "random-1341-S40-N1": 1, "random-1423-S40-N1": 1,
    "random-1522-S40-N1": 1, "random-2121-S40-N1": 1, "random-2135-S40-N63": 6, "random-2164-S40-N63": 7,
    "random-2187-S40-N63": 16, "random-20013-S40-N63": 10, "random-2240-S40-N64": 6, "random-2254-S40-N64": 13,
    "random-2266-S40-N64": 11, "random-20029-S40-N64": 4, "random-2341-S40-N65": 4, "random-2357-S40-N65": 4,
    "random-2359-S40-N65": 16, "random-2413-S40-N700": 181, "random-2438-S40-N700": 66, "random-2444-S40-N700": 47,
    "random-2445-S40-N5000": 512, "random-2448-S40-N5000": 589, "random-2451-S40-N5000": 346, "random-4374-S300-N1": 1,
    "random-4941-S300-N1": 1, "random-5703-S300-N1": 1, "random-6710-S300-N1": 1, "random-6841-S300-N63": 11,
    "random-6895-S300-N63": 6, "random-6924-S300-N63": 7, "random-7004-S300-N64": 21, "random-7017-S300-N64": 11,
    "random-7052-S300-N64": 5, "random-7075-S300-N65": 4, "random-7372-S300-N65": 4, "random-7410-S300-N65": 6,
    "random-7781-S300-N700": 38, "random-8453-S300-N700": 35, "random-9221-S300-N700": 40, "random-10140-S300-N5000": 265,
}


@functools.lru_cache(maxsize=None)
def get(key):
    """The case named `key` — a made case's name, or a (seed, servants, requests) spec —, built once."""
    if isinstance(key, tuple):
        return random_case(*key)
    return {f.__name__: f for f in MADE}[key]()
