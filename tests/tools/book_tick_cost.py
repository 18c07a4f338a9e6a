"""What the running-task book adds to a leased tick, at lease_tick_cost.py's shape:
cfg5's registry, 10k requests, 10k frees by id, 200 heartbeats, 2k renewals and 200 reports per
tick; a grant lives ten ticks, so a reporting servant lists about 50 ids. Streams without and with
a book alternate in one process (two runs each), fed the same ticks; with a book the payload columns
are staged every tick.
    python tests/tools/book_tick_cost.py --ticks 300
prints one JSON line: the median wall time per tick (host call to host return, the staging call
included) of every run. Under `rocprofv3 --kernel-trace --stats -- python
tests/tools/book_tick_cost.py ...` the kernel table gives k_book_commit's share. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS, LIFE = 10_000, 200, 2_000, 10
E64 = np.empty(0, np.uint64)


def run(sv, abi, ticks, max_book):
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    ctx.stream_begin_leased(es.hb + 8, N, N, (LIFE + 4) * N, RENEWALS, N, HB_REPORTS, 1 << 16)
    if max_book:
        ctx.stream_book_begin(max_book)
    rng = np.random.default_rng(5)
    live = []  # (ids, servants) of the last LIFE ticks' grants
    dt, n_ids = [], 0
    for t in range(ticks + 20):
        now = t + 1
        who, rows, rel, tk = es.next_tick()
        fr = live.pop(0)[0] if len(live) == LIFE else E64
        ids_all = np.concatenate([a for a, _ in live]) if live else E64
        srv_all = np.concatenate([b for _, b in live]) if live else np.empty(0, np.uint32)
        ren = rng.choice(ids_all, RENEWALS) if len(ids_all) else E64
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % es.n).astype(np.uint32)
        order = np.argsort(srv_all, kind="stable")
        srt = srv_all[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([ids_all[order[l:h]] for l, h in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        n_ids = len(rid)
        lex = np.full(len(tk["env_id"]), now + 4 * LIFE, np.int64)
        t0 = time.perf_counter()
        if max_book:
            ctx.stream_book_stage(rid + np.uint64(1), rid ^ np.uint64(0x5555))
        out, ids, _, unknown, n_l = ctx.stream_tick_leased(who, rows, rel, ren, np.full(len(ren), now + 4 * LIFE, np.int64),
                                                           fr, rs, off, rid, tk, lex, now)
        dt.append(time.perf_counter() - t0)
        es.commit(out)
        g = out < binding.IDX_ENV_NOT_FOUND
        live.append((ids[g], out[g]))
    n_book = len(ctx.stream_book()[0]) if max_book else 0
    ctx.stream_end()
    ctx.close()
    return round(float(np.median(dt[20:])) * 1e6, 1), n_ids, n_book, int(n_l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--max-book", type=int, default=1 << 18)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    res = {"ticks": a.ticks, "max_book": a.max_book, "plain_leased_tick_us": [], "booked_tick_us": []}
    for max_book in (0, a.max_book, 0, a.max_book):
        us, n_ids, n_book, n_l = run(sv, abi, a.ticks, max_book)
        res["booked_tick_us" if max_book else "plain_leased_tick_us"].append(us)
        res.update(reported_ids_last_tick=n_ids, leases=n_l)
        if max_book:
            res["book_entries"] = n_book
    print(json.dumps(res))


if __name__ == "__main__":
    main()
