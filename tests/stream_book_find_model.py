"""The book by digest (ydc_stream_book_find / ydc_stream_book_distinct) as the reference's daemon
computes it: RunningTaskKeeper::Refresh (running_task_keeper.cc:55-60) makes one pass over the list
GetRunningTasks returned, m[task_digest] = entry, so the last entry of a digest wins; TryFindTask
(:67-75) asks that map. A count per key rides beside it. The yardstick of
tests/test_stream_book_find_gpu.py, pinned against a plain scan by tests/test_stream_book_find_model.py.

`columns` is what tests/stream_book_model.py's Book.columns() returns: (servant_idx, task_grant_id,
servant_task_id, digest_key), in B's order.
"""
import numpy as np

NOT_FOUND = 0xFFFFFFFF  # YDC_BOOK_NOT_FOUND
HIT = np.dtype([("pos", "<u4"), ("count", "<u4"), ("servant_idx", "<u4"), ("reserved", "<u4"),
                ("task_grant_id", "<u8"), ("servant_task_id", "<u8")])  # ydc_book_hit
MISS = (NOT_FOUND, 0, 0, 0, 0, 0)


def refresh(columns):
    """The pass in list order: key -> position of the entry that won, key -> entries seen."""
    m, count = {}, {}
    for p, key in enumerate(columns[3].tolist()):
        m[key] = p
        count[key] = count.get(key, 0) + 1
    return m, count


def find(columns, keys):
    """ydc_stream_book_find: a HIT row per key."""
    srv, gid, stid, _ = columns
    m, count = refresh(columns)
    out = np.zeros(len(keys), HIT)
    for i, key in enumerate(np.asarray(keys, np.uint64).tolist()):
        p = m.get(key)
        out[i] = MISS if p is None else (p, count[key], srv[p], 0, gid[p], stid[p])
    return out


def distinct(columns):
    """ydc_stream_book_distinct: (servant_idx, task_grant_id, servant_task_id, digest_key, count), one
    row per key of the map, ordered by the winning entries' positions."""
    srv, gid, stid, dkey = columns
    m, count = refresh(columns)
    won = np.array(sorted(m.values()), np.int64)
    return (srv[won].astype(np.uint32), gid[won].astype(np.uint64), stid[won].astype(np.uint64),
            dkey[won].astype(np.uint64), np.array([count[k] for k in dkey[won].tolist()], np.uint32))
