"""The state of the stream models (tests/stream_lease_model.py and the models built on it) in the
shape yadcc_amd.snapshot.parse returns and snapshot.build takes: what ydc_stream_snapshot must write
for a context in that state, and what ydc_stream_restore can be handed instead of a C-made blob.

The models keep no report stamps (a stamp only matters inside the tick that made it: k_lease_sweep
compares it with the tick's own number) and no per-servant report tick (the same), so a state built
here carries zeros for both, and `same` does not compare them."""
import numpy as np

from yadcc_amd import snapshot as S

REGISTRY = ("version", "num_processors", "current_load", "servant_max_tasks", "flags", "ip_id", "running_tasks", "env_mask")
SECTIONS = {
    "registry": REGISTRY + ("alias_ip", "alias_servant"),
    "L": ("l_id", "l_servant", "l_expires_at", "l_zombie"),
    "W": ("w_env_id", "w_min_version", "w_requestor_ip", "w_deadline", "w_tag", "w_lease_for", "w_n_immediate",
          "w_n_prefetch"),
    "B": ("b_servant", "b_grant_id", "b_servant_task_id", "b_digest_key"),
    "E": ("e_expires_at",),
    "header": S.CAPS + ("max_book", "next_id", "last_now", "lease_tick", "n_wait_rows", "alive_bound", "n_servants",
                        "env_words") + tuple(name for name, _ in S.MODE_BITS),
}


def state_of(mode, ws, caps, ticks, book=None, alive=None, max_book=0, aliases=((), ())):
    """mode: "leased" | "wait_leased" | "rpc"; ws: the model's stream; caps: the ten bounds (dict,
    ydc_stream_caps' names); ticks: accepted ticks so far (the tick number); book: a
    stream_book_model.Book or None; alive: a stream_alive_model.Alive or None."""
    es, T = ws.es, ws.table
    n = es.n
    d = {k: int(caps.get(k, 0)) for k in S.CAPS}
    d.update(waiting=mode != "leased", leased=True, rpc=mode == "rpc", book=book is not None, alive=alive is not None,
             max_book=int(max_book), next_id=int(T.next_id), lease_tick=int(ticks),
             last_now=S.I64_MIN if T.last_now is None else int(T.last_now))
    env = np.asarray(es.abi["env_mask"], np.uint64).reshape(n, -1)
    d.update(env_mask=env, version=es.sv["version"].astype(np.uint32), num_processors=es.sv["num_processors"].astype(np.uint32),
             current_load=es.sv["current_load"].astype(np.uint32), servant_max_tasks=es.sv["max_tasks"].astype(np.uint32),
             flags=np.asarray(es.abi["flags"], np.uint32), ip_id=np.asarray(es.abi["ip_id"], np.uint32),
             running_tasks=es.running.astype(np.uint32), alias_ip=np.asarray(aliases[0], np.uint32),
             alias_servant=np.asarray(aliases[1], np.uint32))
    ids, srv, exp, zom = T.snapshot()
    d.update(l_id=ids, l_servant=srv, l_expires_at=exp, l_zombie=zom)
    if mode == "wait_leased":
        q = ws.state.q
        d.update(w_env_id=q.cols["env_id"], w_min_version=q.cols["min_version"], w_requestor_ip=q.cols["requestor_ip"],
                 w_deadline=q.deadline, w_tag=q.tag, w_lease_for=ws.state.lease_for)
    elif mode == "rpc":
        q = ws.state.q
        d.update(w_env_id=q.cols["env_id"], w_min_version=q.cols["min_version"], w_requestor_ip=q.cols["requestor_ip"],
                 w_deadline=q.deadline, w_tag=q.tag, w_lease_for=q.lease_for, w_n_immediate=q.cols["n_imm"],
                 w_n_prefetch=q.cols["n_pre"], n_wait_rows=q.rows())
    if book is not None:
        bs, bg, bt, bd = book.columns()
        d.update(b_servant=bs, b_grant_id=bg, b_servant_task_id=bt, b_digest_key=bd)
    if alive is not None:
        d.update(e_expires_at=alive.expires.astype(np.int64),
                 alive_bound=int(alive.expires.min()) if len(alive.expires) else S.I64_MAX)
    return d


def same(parsed, want, sections=("header", "registry", "L", "W", "B", "E")):
    """parse(blob) equals the model's state, section by section."""
    for sec in sections:
        for k in SECTIONS[sec]:
            if k not in want:
                assert k not in parsed or sec == "header", "the blob has a column %s the state lacks" % k
                continue
            a, b = np.asarray(parsed[k]), np.asarray(want[k])
            assert a.shape == b.shape, "%s: %s has shape %s, the model %s" % (sec, k, a.shape, b.shape)
            assert np.array_equal(a, b), "%s: %s differs" % (sec, k)
