"""Cost of a waiting + leased streaming tick beside the plain, the waiting and the leased tick of
the same build in the same process, at the cfg5 shape of tests/tools/lease_tick_cost.py: 2000
servants, 10k requests, 10k frees by id, 200 heartbeats, 200 reports, 2k renewals per tick,
max_waiting 20k, about |L| leases in the table (ballast filled first).
    python tests/tools/wait_lease_tick_cost.py --leases 20000 --ticks 300
prints one JSON line: median wall time per tick (host call to host return) of the four modes, and
what two separate passes would cost: the leased tick plus the waiting tick's surcharge over the
plain one. Under `rocprofv3 --kernel-trace --stats -- python tests/tools/wait_lease_tick_cost.py
...` the kernel table gives k_wait_lease_commit beside k_wait_compact and k_lease_grant. Needs the
GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS, MAX_WAITING = 10_000, 200, 2_000, 20_000
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
FAR = 1 << 40


def plain_or_waiting(sv, abi, ticks, waiting):
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, N)
    ctx.stream_begin(es.hb + 8, N, N, max_waiting=MAX_WAITING if waiting else 0)
    cost, tags = [], np.arange(N, dtype=np.uint64)
    for t in range(ticks + 20):
        who, rows, rel, tk = es.next_tick()
        dl = np.full(N, t + 5, np.int64)
        t0 = time.perf_counter()
        if waiting:
            out, _, ri, _ = ctx.stream_tick_waiting(who, rows, rel, tk, dl, tags, t)
        else:
            out, ri = ctx.stream_tick(who, rows, rel, tk), E32
        cost.append(time.perf_counter() - t0)
        got = np.concatenate([ri, out])
        es.commit(got[got < binding.IDX_WAITING])
    ctx.stream_end()
    ctx.close()
    return cost


def leased(sv, abi, ticks, leases, waiting, rng):
    """The leased tick (waiting: the waiting + leased one) with `leases` ballast leases in L."""
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    max_leases = leases + 4 * N + (MAX_WAITING if waiting else 0)
    if waiting:
        ctx.stream_begin_waiting_leased(es.hb + 8, N, N, MAX_WAITING, max_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    else:
        ctx.stream_begin_leased(es.hb + 8, N, N, max_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    tags = np.arange(N, dtype=np.uint64)

    def tick(who, rows, rel, ren, ren_exp, fr, rs, off, rid, tk, lease_for, now):
        """-> (out, ids, |L|); a grant's lease ends at now + lease_for in both modes."""
        n = len(tk["env_id"])
        if waiting:
            r = ctx.stream_tick_waiting_leased(who, rows, rel, ren, ren_exp, fr, rs, off, rid, tk,
                                               np.full(n, lease_for, np.int64), np.full(n, now + 5, np.int64),
                                               tags[:n], now)
        else:
            r = ctx.stream_tick_leased(who, rows, rel, ren, ren_exp, fr, rs, off, rid, tk,
                                       np.full(n, now + lease_for, np.int64), now)
        return r[0], r[1], r[4]

    held = 0
    while held < leases:  # ballast: leases nobody frees; their slots go back by servant index
        who, rows, _, tk = es.next_tick()
        out, _, held = tick(who, rows, E32, E64, I64, E64, E32, Z1, E64, tk, FAR, 0)
        g = out[out < binding.IDX_WAITING]
        tick(E32, rows[:0], g, E64, I64, E64, E32, Z1, E64, {k: v[:0] for k, v in tk.items()}, FAR, 0)
    live_ids, live_srv, cost = E64, E32, []
    for t in range(ticks + 20):
        now = t + 1
        who, rows, _, tk = es.next_tick()
        ren = rng.integers(0, max(held, 1), RENEWALS).astype(np.uint64)  # ballast ids: live, never freed
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % es.n).astype(np.uint32)
        # every reporting servant lists the grants of the last tick it still holds
        order = np.argsort(live_srv, kind="stable")
        srt = live_srv[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([live_ids[order[l:h]] for l, h in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        t0 = time.perf_counter()
        out, ids, n_l = tick(who, rows, E32, ren, np.full(RENEWALS, FAR, np.int64), live_ids, rs, off, rid, tk, 5, now)
        cost.append(time.perf_counter() - t0)
        g = out < binding.IDX_WAITING
        live_ids, live_srv = ids[g], out[g]
    st = ctx.stats()
    ctx.stream_end()
    ctx.close()
    return cost, int(n_l), {k: st[k] for k in ("granted", "leases_freed", "renewals_refused")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=20_000)
    ap.add_argument("--ticks", type=int, default=300)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    us = lambda v: round(float(np.median(v[20:])) * 1e6, 1)
    plain = us(plain_or_waiting(sv, abi, a.ticks, False))
    wait = us(plain_or_waiting(sv, abi, a.ticks, True))
    lc, n_l, _ = leased(sv, abi, a.ticks, a.leases, False, np.random.default_rng(5))
    cc, n_c, last = leased(sv, abi, a.ticks, a.leases, True, np.random.default_rng(5))
    print(json.dumps({"leases": n_l, "leases_combined": n_c, "ticks": a.ticks, "plain_tick_us": plain,
                      "waiting_tick_us": wait, "leased_tick_us": us(lc), "waiting_leased_tick_us": us(cc),
                      "two_passes_would_cost_us": round(us(lc) + wait - plain, 1), "last_tick": last}))


if __name__ == "__main__":
    main()
