"""A plain reference for placement by ADDRESS STRINGS (test infrastructure, not product code).

The reference scheduler compares a requestor's address with a servant's observed location as
strings (IsNetworkAddressEqual, task_dispatcher.cc:66-69): the location starts with the address and
the next character is ':'. A location with several ':' therefore answers to several addresses
("[::1]:8335" to "[::1]", "[:" and "["). The device API carries that as one host id per servant
(`ip_id`) plus further (host id, servant row) pairs (ydc_set_host_aliases).

This file restates the reference literally and sequentially, on the strings, and does its own
interning of strings into ids. It shares no code with dispatch_core.h, host_tables.h, the C oracle
or gpu_task_dispatcher.cc.

    dispatch(locations, sv, requestors, tk)    one WaitForStartingNewTask(timeout = now) per request
    intern(locations, requestors)              strings -> (primary ids, alias pairs, requestor ids)
"""
import numpy as np

IDX_TIMEOUT = 0xFFFFFFFF
IDX_ENV_NOT_FOUND = 0xFFFFFFFE
PRIORITY_DEDICATED = 1
MIN_MEMORY_DEFAULT = 10 << 30  # --servant_min_memory_for_accepting_new_task=10G (task_dispatcher.cc:35)


def is_network_address_equal(ip_port, ip2):
    """task_dispatcher.cc:66-69, character for character."""
    return len(ip_port) > len(ip2) and ip_port[len(ip2)] == ":" and ip_port.startswith(ip2)


def is_primary_address(ip_port, ip2):
    """What remains of the comparison when the aliases are stripped: only the longest matching
    address, i.e. everything in front of the LAST ':'."""
    return is_network_address_equal(ip_port, ip2) and ":" not in ip_port[len(ip2) + 1:]


def capacity_available(nproc, load, max_tasks, total_memory, memory_available, running, min_memory):
    """GetCapacityAvailable, task_dispatcher.cc:283-313."""
    if total_memory and memory_available < min_memory:  # :286-292
        return running
    foreign_load = max(load - running, 0)                # :308-309
    capacity = max(nproc - foreign_load, 0)              # :310-311
    return min(max_tasks, capacity)                      # :312


def _has_env(mask_row, env):
    """Digest `env` is bit env % 64 of word env / 64 of the servant's environment set."""
    words = [int(mask_row)] if np.ndim(mask_row) == 0 else [int(w) for w in mask_row]
    return env // 64 < len(words) and bool(words[env // 64] >> (env % 64) & 1)


def dispatch(locations, sv, requestors, tk, running=None, same_host=is_network_address_equal,
             min_memory=MIN_MEMORY_DEFAULT, fallbacks=None):
    """locations: per servant its observed location; sv: the raw servant columns (version,
    num_processors, current_load, max_tasks, running_tasks, priority, total_memory, memory_available,
    env_mask); requestors: per request the requestor's address; tk: env_id and min_version columns.
    running: the running_tasks to start from (default: sv's). same_host: the address comparison.
    fallbacks: a list that receives the requests granted their own servant (:392-396).
    Returns (servant index or IDX_* per request as uint32, utilisation per request as float64 with
    -1.0 where nothing was granted, running_tasks afterwards as uint32)."""
    S = len(locations)
    col = lambda k: [int(x) for x in sv[k]]
    version, nproc, load, max_tasks = col("version"), col("num_processors"), col("current_load"), col("max_tasks")
    priority, total_memory, memory_available = col("priority"), col("total_memory"), col("memory_available")
    running = [int(x) for x in (sv["running_tasks"] if running is None else running)]
    env_mask = sv["env_mask"]
    N = len(requestors)
    out = np.empty(N, np.uint32)
    util_out = np.empty(N, np.float64)
    eligible_of = {}  # (digest, min_version) -> eligible servants: the registry does not change in a batch

    def cap(s):
        return capacity_available(nproc[s], load[s], max_tasks[s], total_memory[s], memory_available[s],
                                  running[s], min_memory)

    for t in range(N):
        env, minv, requestor = int(tk["env_id"][t]), int(tk["min_version"][t]), requestors[t]
        # UnsafeEnumerateEligibleServants, :316-344
        eligibles = eligible_of.get((env, minv))
        if eligibles is None:
            eligibles = [s for s in range(S)
                         if _has_env(env_mask[s], env) and max_tasks[s] != 0 and not version[s] < minv]
            eligible_of[(env, minv)] = eligibles
        if not eligibles:
            out[t], util_out[t] = IDX_ENV_NOT_FOUND, -1.0
            continue
        # UnsafeEnumerateFreeServants, :346-360
        servants = [s for s in eligibles if not running[s] >= cap(s)]
        if not servants:
            out[t], util_out[t] = IDX_TIMEOUT, -1.0
            continue
        # UnsafePickServantFor, :362-397
        self = None
        for i, s in enumerate(servants):  # :373-375: the FIRST of the list, registry order
            if same_host(locations[s], requestor):
                self = s
                del servants[i]           # :378
                break
        pick = None
        for dedicated_only in (True, False):  # :382-390
            result, min_utilization = None, None
            for s in servants:                # UnsafeTryPickServantFor, :417-451
                if dedicated_only and not (priority[s] == PRIORITY_DEDICATED and running[s] * 2 < nproc[s]):
                    continue
                utilization = float(running[s]) / cap(s)
                if result is None or utilization < min_utilization:  # :444, strict
                    min_utilization, result = utilization, s
            if result is not None:
                pick, u = result, min_utilization
                break
        if pick is None:  # :392-396
            assert self is not None and cap(self) != 0
            pick, u = self, float(running[self]) / cap(self)
            if fallbacks is not None:
                fallbacks.append(t)
        running[pick] += 1
        out[t], util_out[t] = pick, u
    return out, util_out, np.array(running, np.uint32)


def _ids(start=1, step=0x9E3779B1, offset=0x7F4A7C15):
    """Distinct 32-bit ids, scattered over the whole range (an odd multiplier permutes 2^32)."""
    k = start
    while True:
        v = (k * step + offset) & 0xFFFFFFFF
        k += 1
        if v < 0xFFFFFF00:
            yield v


def intern(locations, requestors):
    """-> (primary[S] uint32, (alias_ip, alias_servant) uint32 columns, requestor_id[len(requestors)]
    uint32, names: address string -> id).
    Primary id of a servant: the id of the longest address it answers to, everything in front of
    its last ':'; a location without ':' answers to nobody and gets an id of its own. Alias pairs:
    (id of a shorter address, servant). A requestor's id is the id of its string if some location
    answers to it, otherwise an id that belongs to no servant (one per distinct string)."""
    fresh = _ids()
    names = {}
    primary = np.empty(len(locations), np.uint32)
    alias_ip, alias_servant = [], []
    for s, loc in enumerate(locations):
        cuts = [i for i, ch in enumerate(loc) if ch == ":"]
        if not cuts:
            primary[s] = next(fresh)
            continue
        for i in cuts:
            if loc[:i] not in names:
                names[loc[:i]] = next(fresh)
        primary[s] = names[loc[:cuts[-1]]]
        for i in cuts[:-1]:
            alias_ip.append(names[loc[:i]])
            alias_servant.append(s)
    strangers = {}
    rid = np.empty(len(requestors), np.uint32)
    for t, r in enumerate(requestors):
        if r in names:
            rid[t] = names[r]
        else:
            if r not in strangers:
                strangers[r] = next(fresh)
            rid[t] = strangers[r]
    return primary, (np.array(alias_ip, np.uint32), np.array(alias_servant, np.uint32)), rid, names
