"""ydc_stream_inspect_select / ydc_stream_inspect_count as a plain model: the yardstick of
tests/test_stream_select_gpu.py, with hand cases of its own in tests/test_stream_select_model.py.

Written from the call's semantics and nothing else: T is what Inspect.tasks() of
tests/stream_inspect_model.py answers (with inspection off: the lease model's table with the sentinel
details), a filter is a set of keywords, the answer is the filtered T cut at `cap` rows, in T's
ascending id order, beside the number of rows that satisfy the filter. It shares no code with the
library: the filter is a column-wise mask here, a per-row conjunction there.
"""
import numpy as np

NO_ID = 0xFFFFFFFF
NO_TIME = -(1 << 63)
COLS = ("task_id", "servant_idx", "expires_at", "zombie", "started_at", "env_id", "requestor_ip", "prefetch")
DTYPES = (np.uint64, np.uint32, np.int64, np.uint8, np.int64, np.uint32, np.uint32, np.uint8)
TABLE_KEYS = ("servant", "zombie", "expires_before", "after_id")
RECORD_KEYS = ("env_id", "requestor_ip", "prefetch", "started_before")
KEYS = TABLE_KEYS + RECORD_KEYS + ("unattributed",)


def table(ws, inspect=None):
    """T of the stream `ws`: with inspection its Inspect's tasks(), without it the lease table in id
    order with the sentinels beside it."""
    if inspect is not None:
        return inspect.tasks()
    ids, srv, exp, zom = ws.table.snapshot()
    n = len(ids)
    return {"task_id": ids, "servant_idx": srv, "expires_at": exp, "zombie": zom,
            "started_at": np.full(n, NO_TIME, np.int64), "env_id": np.full(n, NO_ID, np.uint32),
            "requestor_ip": np.full(n, NO_ID, np.uint32), "prefetch": np.zeros(n, np.uint8)}


def rows(cols):
    """T from literal rows (id, servant, expires_at, zombie, started_at, env_id, requestor_ip, prefetch),
    sorted by id."""
    cols = sorted(cols)
    return {k: np.array([r[i] for r in cols], t) for i, (k, t) in enumerate(zip(COLS, DTYPES))}


def mask(T, servant=None, zombie=None, expires_before=None, after_id=None, env_id=None, requestor_ip=None,
         prefetch=None, started_before=None, unattributed=False):
    """Which rows of T satisfy the filter. Python integers throughout: no value wraps."""
    n = len(T["task_id"])
    col = lambda k: [int(v) for v in T[k]]
    keep = [True] * n
    def also(values, test):
        for i, v in enumerate(values):
            keep[i] = keep[i] and test(v)
    if servant is not None:
        also(col("servant_idx"), lambda v: v == int(servant))
    if zombie is not None:
        also(col("zombie"), lambda v: v == int(zombie))
    if expires_before is not None:
        also(col("expires_at"), lambda v: v < int(expires_before))
    if after_id is not None:
        also(col("task_id"), lambda v: v > int(after_id))
    record = [v is not None for v in (env_id, requestor_ip, prefetch, started_before)]
    if unattributed:
        also(col("started_at"), lambda v: v == NO_TIME and not any(record))
    elif any(record):
        also(col("started_at"), lambda v: v != NO_TIME)
    if env_id is not None:
        also(col("env_id"), lambda v: v == int(env_id))
    if requestor_ip is not None:
        also(col("requestor_ip"), lambda v: v == int(requestor_ip))
    if prefetch is not None:
        also(col("prefetch"), lambda v: v == int(prefetch))
    if started_before is not None:
        also(col("started_at"), lambda v: v < int(started_before))
    return np.array(keep, bool)


def select(T, cap, **flt):
    """-> (the first min(matches, cap) matching rows of T as a dict of columns, matches)."""
    assert list(T["task_id"]) == sorted(int(t) for t in T["task_id"])
    at = sorted(np.nonzero(mask(T, **flt))[0].tolist(), key=lambda i: int(T["task_id"][i]))
    return {k: T[k][at[:cap]] for k in COLS}, len(at)


def count(T, filters):
    return np.array([int(mask(T, **f).sum()) for f in filters], np.uint32)


def pages(T, page, **flt):
    """The pages a caller gets who repeats the call with the cursor: a list of column dicts."""
    out = []
    while True:
        cols, matches = select(T, page, **flt)
        n = len(cols["task_id"])
        if n:
            out.append(cols)
        if matches <= n:
            return out
        flt["after_id"] = int(cols["task_id"][-1])


def concat(pgs):
    return {k: np.concatenate([p[k] for p in pgs]) if pgs else np.empty(0, t) for k, t in zip(COLS, DTYPES)}


def same(got, want, what=""):
    for k in COLS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, "%s: %s: row %d gpu %s model %s (%d differ)" % (what, k, bad[0], got[k][bad[0]],
                                                                             want[k][bad[0]], bad.size)


def random_filter(T, rng, now):
    """A filter drawn from T's own values, so that most filters match something: 0 - 2 predicates
    (3 now and then), each value taken from a row of T picked at random (thresholds one above that row's
    value, so that the row itself passes). An empty T draws the empty filter."""
    n = len(T["task_id"])
    if n == 0:
        return {}
    i = int(rng.integers(n))
    attributed = int(T["started_at"][i]) != NO_TIME
    draw = {"servant": lambda: int(T["servant_idx"][i]), "zombie": lambda: int(T["zombie"][i]),
            "expires_before": lambda: int(T["expires_at"][i]) + 1 + int(rng.integers(0, 30)),
            "after_id": lambda: max(int(T["task_id"][int(rng.integers(0, i + 1))]) - 1, 0)}  # (below row i's id)
    if attributed:
        draw.update({"env_id": lambda: int(T["env_id"][i]), "requestor_ip": lambda: int(T["requestor_ip"][i]),
                     "prefetch": lambda: int(T["prefetch"][i]),
                     "started_before": lambda: int(T["started_at"][i]) + 1 + int(rng.integers(0, 5))})
    else:
        draw["unattributed"] = lambda: True
    k = int(rng.choice([0, 1, 1, 1, 2, 2, 3]))
    names = sorted(draw)
    picked = [names[j] for j in rng.permutation(len(names))[:k]]
    return {name: draw[name]() for name in picked}
