"""The outlook per request personality (ydc_stream_outlook_get) and the view of the waiting queue
(ydc_stream_inspect_waiting) as a plain numpy model: the yardstick of tests/test_stream_outlook_gpu.py,
pinned against the verbatim reference by tests/test_stream_outlook_model.py.

It reads what the other models keep and edits none of them: a registry snapshot (the stream's `sv`
columns, its flags and its running_tasks), the queue of the wait / wait-and-lease / rpc model, and
the lease model's table with stream_inspect_model's records.

Supply, for a personality (env_id, min_version):
  eligible            servants with max_tasks != 0, bit env_id in their environment set and
                      version >= min_version (UnsafeEnumerateEligibleServants, task_dispatcher.cc:316-344)
  free_servants       of those, running_tasks < GetCapacityAvailable (:346-360)
  grants_available    sum over the eligible of grants(): how often the grant call succeeds on one
                      servant in a row (every grant adds 1 to running_tasks, :123). Capacity GROWS
                      with running_tasks while current_load covers them (:308-311), so this is not
                      capacity_available - running_tasks; grants_by_rule() applies :354 literally, grants()
                      is the closed form (free(r) <=> not low memory, load < nproc, r < min(max_tasks,
                      nproc)), and the model test holds one against the other.
  running_tasks, max_tasks, capacity_available    sums over the eligible.
Demand, by env_id alone: waiting / waiting_rows over W, leases / zombies over the inspection records.
"""
import numpy as np

from tests.stream_inspect_model import LOW_MEMORY, capacity

UNKNOWN = 0xFFFFFFFF  # YDC_OUTLOOK_UNKNOWN
NO_ID = 0xFFFFFFFF    # YDC_INSPECT_NO_ID
COLUMNS = ("eligible", "free_servants", "grants_available", "running_tasks", "max_tasks", "capacity_available",
           "waiting", "waiting_rows", "leases", "zombies")
DTYPES = dict(eligible=np.uint32, free_servants=np.uint32, grants_available=np.uint64, running_tasks=np.uint64,
              max_tasks=np.uint64, capacity_available=np.uint64, waiting=np.uint32, waiting_rows=np.uint32,
              leases=np.uint32, zombies=np.uint32)
WAITING_COLUMNS = ("tag", "env_id", "min_version", "requestor_ip", "deadline", "lease_for", "n_immediate", "n_prefetch")


def grants_by_rule(nproc, load, max_tasks, running, low_memory, limit=1 << 12):
    """Grants one servant gives in a row: :354 before each, :123 after each."""
    r, n = int(running), 0
    while r < capacity(nproc, load, max_tasks, r, low_memory):
        r, n = r + 1, n + 1
        assert n < limit
    return n


def grants(nproc, load, max_tasks, running, low_memory):
    """The closed form of grants_by_rule (dispatch_core.h: servant_slot_count)."""
    if low_memory or int(max_tasks) == 0 or int(load) >= int(nproc):
        return 0
    return max(min(int(max_tasks), int(nproc)) - int(running), 0)


def env_words(sv):
    em = sv["env_mask"]
    return em.shape[1] if em.ndim == 2 else 1


def has_env(sv, env):
    """Per servant: whether its environment set has bit `env` (False for a digest nobody can have)."""
    em = np.asarray(sv["env_mask"], np.uint64)
    if em.ndim == 1:
        em = em[:, None]
    if env >= 64 * em.shape[1]:
        return np.zeros(len(em), bool)
    return ((em[:, env // 64] >> np.uint64(env % 64)) & np.uint64(1)).astype(bool)


def outlook(sv, flags, running, env_id, min_version, queue=None, leases=None):
    """sv: the registry's columns; flags: its YDC_SERVANT_* flags; running: running_tasks.
    queue: None (a stream without W) or (env_id, rows) per entry of W. leases: None (inspection off)
    or (env_id, zombie) per lease of L. -> dict of COLUMNS, one row per query."""
    n = len(env_id)
    out = {k: np.zeros(n, DTYPES[k]) for k in COLUMNS}
    S = len(sv["version"])
    low = (np.asarray(flags, np.uint32) & LOW_MEMORY) != 0
    run = np.asarray(running, np.int64)
    per = [(capacity(sv["num_processors"][s], sv["current_load"][s], sv["max_tasks"][s], run[s], low[s]),
            grants(sv["num_processors"][s], sv["current_load"][s], sv["max_tasks"][s], run[s], low[s]))
           for s in range(S)]
    cap = np.array([p[0] for p in per], np.int64)
    slots = np.array([p[1] for p in per], np.int64)
    maxt = np.asarray(sv["max_tasks"], np.int64)
    bins = 64 * env_words(sv)
    for q in range(n):
        e, mv = int(env_id[q]), int(min_version[q])
        el = (maxt != 0) & has_env(sv, e) & (np.asarray(sv["version"], np.int64) >= mv) if S else np.zeros(0, bool)
        out["eligible"][q] = int(el.sum())
        out["free_servants"][q] = int((el & (run < cap)).sum())
        out["grants_available"][q] = sum(int(v) for v in slots[el])
        out["running_tasks"][q] = sum(int(v) for v in run[el])
        out["max_tasks"][q] = sum(int(v) for v in maxt[el])
        out["capacity_available"][q] = sum(int(v) for v in cap[el])
        known = e < bins
        if queue is not None and known:
            mine = np.asarray(queue[0], np.int64) == e
            out["waiting"][q] = int(mine.sum())
            out["waiting_rows"][q] = int(np.asarray(queue[1], np.int64)[mine].sum())
        if leases is None:
            out["leases"][q] = out["zombies"][q] = UNKNOWN
        elif known:
            mine = np.asarray(leases[0], np.int64) == e
            out["leases"][q] = int(mine.sum())
            out["zombies"][q] = int((np.asarray(leases[1]) != 0)[mine].sum())
    return out


def waiting(q, lease_for=None):
    """W as ydc_stream_inspect_waiting returns it, from a model's queue: a stream_wait_model.WaitQueue
    (lease_for: the wait-and-lease state's sixth column, None in waiting mode), a
    stream_rpc_model.RpcQueue, or None (a leased stream: no W)."""
    if q is None:
        z32, z64 = np.empty(0, np.uint32), np.empty(0, np.int64)
        return dict(tag=np.empty(0, np.uint64), env_id=z32, min_version=z32, requestor_ip=z32, deadline=z64,
                    lease_for=z64, n_immediate=z32, n_prefetch=z32)
    n = len(q.tag)
    rpc = "n_imm" in q.cols
    if rpc:
        lease_for = q.lease_for
    return dict(tag=q.tag.astype(np.uint64), env_id=q.cols["env_id"].astype(np.uint32),
                min_version=q.cols["min_version"].astype(np.uint32), requestor_ip=q.cols["requestor_ip"].astype(np.uint32),
                deadline=q.deadline.astype(np.int64),
                lease_for=np.zeros(n, np.int64) if lease_for is None else np.asarray(lease_for, np.int64),
                n_immediate=q.cols["n_imm"].astype(np.uint32) if rpc else np.ones(n, np.uint32),
                n_prefetch=q.cols["n_pre"].astype(np.uint32) if rpc else np.zeros(n, np.uint32))


def queue_of(ws):
    """The queue and its lease_for column of a model stream of any mode: (q, lease_for)."""
    st = getattr(ws, "state", None)
    if st is None:
        return None, None
    return st.q, getattr(st, "lease_for", None)


def stream_waiting(ws):
    return waiting(*queue_of(ws))


def stream_outlook(ws, env_id, min_version, inspect=None):
    """The outlook of a lease-model stream `ws` (stream_lease_model.LeaseStream or one built on it) as
    the device must answer it. inspect: its stream_inspect_model.Inspect, None while inspection is off."""
    es = ws.es
    w = stream_waiting(ws)
    queue = None if getattr(ws, "state", None) is None else (w["env_id"], w["n_immediate"].astype(np.int64) + w["n_prefetch"])
    leases = None
    if inspect is not None:
        t = inspect.tasks()
        leases = (t["env_id"], t["zombie"])
    return outlook(es.sv, es.abi["flags"], es.running, env_id, min_version, queue, leases)
