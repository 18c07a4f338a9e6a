"""The load per requestor (ydc_stream_requestor_find / ydc_stream_requestor_get) as a NumPy fold of
what the EXISTING getters answer — the dicts of binding.Context.stream_inspect_tasks() and
stream_waiting(), or the models' equivalents stream_inspect_model.Inspect.tasks() and
stream_outlook_model.stream_waiting() —, and the admission arithmetic (ydc_admit_clip) written as the
literal sequential loop. Nothing here uses the new code. The device is compared with it by
tests/test_stream_requestor_gpu.py; tests/test_stream_requestor_model.py pins the fold against a
dictionary count and the loop against the closed form."""
import numpy as np

UNKNOWN = 0xFFFFFFFF  # YDC_REQUESTOR_UNKNOWN
NO_TIME = -(1 << 63)  # YDC_INSPECT_NO_TIME
DTYPE = np.dtype([("requestor_ip", "<u4"), ("leases", "<u4"), ("zombies", "<u4"), ("prefetch_leases", "<u4"),
                  ("waiting", "<u4"), ("waiting_rows", "<u4")])  # ydc_requestor_load
COLUMNS = DTYPE.names[1:]


def fold(tasks, waiting):
    """-> (rows sorted by requestor_ip, one per requestor with a lease or an entry of W; unattributed).
    tasks: the dict of stream_inspect_tasks, or None (no L, or inspection off): the lease columns
    and `unattributed` are UNKNOWN then. waiting: the dict of stream_waiting, or None (no W)."""
    ips = [np.empty(0, np.uint32)]
    unattributed = UNKNOWN
    if tasks is not None:
        known = np.asarray(tasks["started_at"], np.int64) != NO_TIME
        unattributed = int((~known).sum())
        l_ip = np.asarray(tasks["requestor_ip"], np.uint32)[known]
        l_zombie = (np.asarray(tasks["zombie"]) != 0)[known].astype(np.int64)
        l_pre = np.asarray(tasks["prefetch"], np.int64)[known]
        ips.append(l_ip)
    if waiting is not None:
        w_ip = np.asarray(waiting["requestor_ip"], np.uint32)
        w_rows = np.asarray(waiting["n_immediate"], np.int64) + np.asarray(waiting["n_prefetch"], np.int64)
        ips.append(w_ip)
    keys = np.unique(np.concatenate(ips))
    out = np.zeros(len(keys), DTYPE)
    out["requestor_ip"] = keys
    if tasks is not None:
        at = np.searchsorted(keys, l_ip)
        out["leases"] = np.bincount(at, minlength=len(keys))
        out["zombies"] = np.bincount(at, weights=l_zombie, minlength=len(keys))
        out["prefetch_leases"] = np.bincount(at, weights=l_pre, minlength=len(keys))
    else:
        for k in ("leases", "zombies", "prefetch_leases"):
            out[k] = UNKNOWN
    if waiting is not None:
        at = np.searchsorted(keys, w_ip)
        out["waiting"] = np.bincount(at, minlength=len(keys))
        out["waiting_rows"] = np.bincount(at, weights=w_rows, minlength=len(keys))
    return out, unattributed


def find(rows, ips, lease_columns=True):
    """The rows of `fold` asked by requestor: one row per entry of ips, zeros for a requestor that
    holds nothing (lease columns UNKNOWN without them)."""
    ips = np.asarray(ips, np.uint32)
    out = np.zeros(len(ips), DTYPE)
    out["requestor_ip"] = ips
    if not lease_columns:
        for k in ("leases", "zombies", "prefetch_leases"):
            out[k] = UNKNOWN
    if len(rows):
        at = np.minimum(np.searchsorted(rows["requestor_ip"], ips), len(rows) - 1)
        hit = rows["requestor_ip"][at] == ips
        out[hit] = rows[at[hit]]
    return out


def stream_fold(ws, inspect):
    """The fold of a model stream of any lease mode; inspect: its stream_inspect_model.Inspect, None
    while inspection is off."""
    from tests import stream_outlook_model as OM
    has_w = getattr(ws, "state", None) is not None
    return fold(None if inspect is None else inspect.tasks(), OM.stream_waiting(ws) if has_w else None)


def admit_clip(requestor_ip, n_immediate, n_prefetch, load, cap):
    """The sequential loop: every requestor starts with room = cap - (leases + waiting_rows), never
    below 0; a row takes what is left of its requestor's room, immediate grants first."""
    left = {}
    out_imm, out_pre = [], []
    for i, ip in enumerate(int(x) for x in requestor_ip):
        if int(load[i]["leases"]) == UNKNOWN:
            raise ValueError("a load with unknown lease columns")
        if ip not in left:
            left[ip] = max(int(cap) - (int(load[i]["leases"]) + int(load[i]["waiting_rows"])), 0)
        imm = int(n_immediate[i])
        pre = 0 if n_prefetch is None else int(n_prefetch[i])
        a_imm = min(imm, left[ip])
        left[ip] -= a_imm
        a_pre = min(pre, left[ip])
        left[ip] -= a_pre
        out_imm.append(a_imm)
        out_pre.append(a_pre)
    return np.array(out_imm, np.uint32), np.array(out_pre, np.uint32)


def admit_clip_closed(requestor_ip, n_immediate, n_prefetch, load, cap):
    """The closed form of the header: a_i = min(pre_i + want_i, room) - min(pre_i, room)."""
    pre_sum = {}
    out_imm, out_pre = [], []
    for i, ip in enumerate(int(x) for x in requestor_ip):
        room = max(int(cap) - min(int(cap), int(load[i]["leases"]) + int(load[i]["waiting_rows"])), 0)
        imm = int(n_immediate[i])
        want = imm + (0 if n_prefetch is None else int(n_prefetch[i]))
        p = pre_sum.get(ip, 0)
        a = min(p + want, room) - min(p, room)
        pre_sum[ip] = p + want
        out_imm.append(min(imm, a))
        out_pre.append(a - min(imm, a))
    return np.array(out_imm, np.uint32), np.array(out_pre, np.uint32)
