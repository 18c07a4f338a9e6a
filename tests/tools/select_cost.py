"""Cost of the lease select (ydc_stream_inspect_select / ydc_stream_inspect_count).

A leased stream with inspection on that holds --leases N leases (default 100 000) of 1 000 requestors, one
of them holding 90 % (depart_cost.py's "hot" shape). Each question is asked both ways of the same context:
  select    the call;
  by_hand   what the parent commit offers: ydc_stream_inspect_tasks copies all of L out, a numpy filter by
            requestor_ip, the first rows of the result.
Legs:
  one_cap100    one cold requestor's leases, cap = 100 (everything fits: count pass and pack)
  hot_cap100    the hot requestor's leases, cap = 100 (the radix select runs)
  hot_capM      the hot requestor's leases, cap = M (everything is packed and copied)
  count64       ydc_stream_inspect_count of 64 requestors, against one copy of L and 64 numpy masks
Medians and min / max of --repeats (at least 5), microseconds of wall time from host call to host return
(every call ends in a device synchronise); the two ways alternate inside a repeat. Answers are compared
once per leg, outside the timed region.
    python tests/tools/select_cost.py --leases 1000000
One JSON line per leg. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack  # noqa: E402
from tests.tools.depart_cost import Holder, REQUESTORS, registry, spread, us  # noqa: E402


def by_hand(ctx, ip, cap):
    t = ctx.stream_inspect_tasks()
    at = np.nonzero((t["requestor_ip"] == ip) & (t["started_at"] != binding.INSPECT_NO_TIME))[0]
    return {k: v[at[:cap]] for k, v in t.items()}, len(at)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert a.repeats >= 5
    rng = np.random.default_rng(5)
    ids = ((10 << 24) + 1 + np.arange(REQUESTORS)).astype(np.uint32)
    who = rng.choice(ids[1:], a.leases)
    who[rng.random(a.leases) < 0.9] = ids[0]
    h = Holder(pack.to_abi_columns(registry()), a.leases, 16, False)
    h.grant(who)
    assert h.n_leases == a.leases
    ctx = h.ctx
    hot, cold = int(ids[0]), int(ids[1])
    M = int((who == hot).sum())
    legs = {"one_cap100": (cold, 100), "hot_cap100": (hot, 100), "hot_capM": (hot, M)}
    clock = time.perf_counter
    for name, (ip, cap) in legs.items():
        sel, hand = [], []
        for r in range(a.repeats + 1):  # (the first repeat warms both ways up and is dropped)
            t0 = clock(); got, m = ctx.stream_inspect_select(cap, requestor_ip=ip); t1 = clock()  # noqa: E702
            want, wm = by_hand(ctx, ip, cap); t2 = clock()  # noqa: E702
            sel.append(t1 - t0)
            hand.append(t2 - t1)
        assert m == wm and all(np.array_equal(got[k], want[k]) for k in got), name
        print(json.dumps({"what": name, "leases": a.leases, "matches": m, "rows": len(got["task_id"]), "repeats": a.repeats,
                          "select_us": us(sel[1:]), "select_min_max_us": spread(sel[1:]),
                          "by_hand_us": us(hand[1:]), "by_hand_min_max_us": spread(hand[1:])}), flush=True)
    q = [int(x) for x in ids[:64]]
    cnt, hand = [], []
    for r in range(a.repeats + 1):
        t0 = clock(); got = ctx.stream_inspect_count([{"requestor_ip": ip} for ip in q]); t1 = clock()  # noqa: E702
        t = ctx.stream_inspect_tasks()
        known = t["started_at"] != binding.INSPECT_NO_TIME
        want = np.array([int(((t["requestor_ip"] == ip) & known).sum()) for ip in q], np.uint32); t2 = clock()  # noqa: E702
        cnt.append(t1 - t0)
        hand.append(t2 - t1)
    assert np.array_equal(got, want)
    print(json.dumps({"what": "count64", "leases": a.leases, "filters": 64, "repeats": a.repeats, "select_us": us(cnt[1:]),
                      "select_min_max_us": spread(cnt[1:]), "by_hand_us": us(hand[1:]),
                      "by_hand_min_max_us": spread(hand[1:])}), flush=True)
    h.close()


if __name__ == "__main__":
    main()
