"""The byte format of ydc_stream_snapshot / ydc_stream_restore in numpy: parse(blob)
-> dict of arrays, build(dict) -> bytes. No compute and no library: this is the format's second,
independent implementation (the first is yadcc_amd/csrc/stream_snapshot_codec.h), so a state built
here restores, and a state snapshotted there reads here, only if the two agree on every byte."""
import struct

import numpy as np

MAGIC = 0x3150414E53434459  # "YDCSNAP1"
VERSION = 1
MODE_BITS = (("waiting", 1), ("leased", 2), ("rpc", 4), ("book", 8), ("alive", 16))
CAPS = ("max_updates", "max_releases", "max_tasks", "max_rows", "max_waiting", "max_leases",
        "max_renewals", "max_frees", "max_reports", "max_report_ids")
LIVE, ZOMBIE, STAMP = 1 << 31, 1 << 30, (1 << 30) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
HEADER = struct.Struct("<QIIQQ4I10II4IIQqq10Q")
HEADER_BYTES = 216
CHECKSUM_WORD = 3
assert HEADER.size == HEADER_BYTES

# (the servants' max_tasks column is "servant_max_tasks" here: "max_tasks" is the stream's bound)
REGISTRY_U32 = ("version", "num_processors", "current_load", "servant_max_tasks", "flags", "ip_id", "running_tasks",
                "rep_tick")


class FormatError(ValueError):
    pass


def _pad8(b):
    return (b + 7) & ~7


def _sections(mode, env_words, n, n_alias, n_l, n_w, n_b):
    """[(name, [(column, dtype, count)], bytes)] in the blob's order."""
    leased, rpc = mode & 2, mode & 4
    reg = [("env_mask", "<u8", n * env_words)] + [(k, "<u4", n) for k in REGISTRY_U32] + [
        ("alias_ip", "<u4", n_alias), ("alias_servant", "<u4", n_alias)]
    lcols = [("l_id", "<u8", n_l), ("l_expires_at", "<i8", n_l), ("l_servant", "<u4", n_l),
             ("l_state", "<u4", n_l)] if leased else []
    w = []
    if mode & 1:
        w = [("w_deadline", "<i8", n_w), ("w_tag", "<u8", n_w)] + ([("w_lease_for", "<i8", n_w)] if leased else []) + [
            ("w_env_id", "<u4", n_w), ("w_min_version", "<u4", n_w), ("w_requestor_ip", "<u4", n_w)] + (
                [("w_n_immediate", "<u4", n_w), ("w_n_prefetch", "<u4", n_w)] if rpc else [])
    b = [("b_grant_id", "<u8", n_b), ("b_servant_task_id", "<u8", n_b), ("b_digest_key", "<u8", n_b),
         ("b_servant", "<u4", n_b)] if mode & 8 else []
    e = [("e_expires_at", "<i8", n)] if mode & 16 else []
    out = []
    for name, cols in (("registry", reg), ("L", lcols), ("W", w), ("B", b), ("E", e)):
        out.append((name, cols, _pad8(sum(np.dtype(dt).itemsize * k for _, dt, k in cols))))
    return out


def checksum(blob):
    """Sum over the 8-byte words of mix(word ^ index * phi), the checksum's own word read as 0."""
    w = np.frombuffer(bytes(blob), "<u8").copy()
    w[CHECKSUM_WORD] = 0
    with np.errstate(over="ignore"):
        z = w ^ (np.arange(len(w), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(z.sum(dtype=np.uint64))


def mode_of(d):
    return sum(bit for name, bit in MODE_BITS if d.get(name))


def _check(ok, why):
    if not ok:
        raise FormatError(why)


def parse(blob):
    """The blob as a dict: the header's fields (mode bits as booleans waiting / leased / rpc / book /
    alive, the bounds under ydc_stream_caps' names, max_book, n_servants, env_words, next_id, last_now,
    lease_tick, alive_bound, n_wait_rows), every column under the names of _sections, and l_zombie /
    l_stamp decoded from l_state. Raises FormatError for anything ydc_stream_restore would refuse for
    its bytes alone."""
    blob = bytes(blob)
    _check(len(blob) >= HEADER_BYTES, "shorter than a header")
    f = HEADER.unpack_from(blob)
    magic, version, hbytes, total, csum, mode, env_words, n, n_alias = f[:9]
    caps = dict(zip(CAPS, f[9:19]))
    max_book, n_l, n_w, n_rows, n_b, lease_tick, next_id, last_now, alive_bound = f[19:28]
    directory = f[28:38]
    _check(magic == MAGIC, "not a stream snapshot (magic)")
    _check(version == VERSION, "unknown format version")
    _check(hbytes == HEADER_BYTES, "header size")
    _check(total == len(blob) and total % 8 == 0, "total bytes differ from the block's size")
    _check(mode & ~31 == 0 and mode & 3, "mode bits")
    _check(not (mode & 4) or mode & 3 == 3, "rpc mode without W or L")
    _check(not (mode & 24) or mode & 2, "book or aliveness without L")
    _check(1 <= env_words <= 64, "env_words out of range")
    _check(caps["max_tasks"] > 0, "max_tasks is 0")
    for bit, cap in ((1, caps["max_waiting"]), (2, caps["max_leases"]), (4, caps["max_rows"]), (8, max_book)):
        _check(bool(mode & bit) == bool(cap), "a bound does not fit the mode")
    if not mode & 2:
        _check(not any((caps["max_renewals"], caps["max_frees"], caps["max_reports"], caps["max_report_ids"], n_l,
                        lease_tick, next_id)), "lease fields without L")
    _check(n_l <= caps["max_leases"] and n_w <= caps["max_waiting"] and n_b <= max_book and n_rows <= caps["max_rows"],
           "a count beyond its bound")
    _check(lease_tick == 0 or lease_tick & STAMP, "a tick number whose stamp is 0")
    _check(mode & 16 or alive_bound == I64_MAX, "alive_bound without E")
    d = dict(caps, max_book=max_book, n_servants=n, env_words=env_words, next_id=next_id, last_now=last_now,
             lease_tick=lease_tick, alive_bound=alive_bound, n_wait_rows=n_rows)
    for name, bit in MODE_BITS:
        d[name] = bool(mode & bit)
    off = HEADER_BYTES
    for k, (name, cols, size) in enumerate(_sections(mode, env_words, n, n_alias, n_l, n_w, n_b)):
        _check(directory[2 * k] == off and directory[2 * k + 1] == size, "section %s is not where its counts put it" % name)
        _check(off + size <= len(blob), "section %s reaches past the end" % name)
        p = off
        for col, dt, cnt in cols:
            d[col] = np.frombuffer(blob, dt, cnt, p).copy()
            p += np.dtype(dt).itemsize * cnt
        _check(not any(blob[p:off + size]), "padding is not zero")
        off += size
    _check(off == len(blob), "bytes behind the last section")
    _check(checksum(blob) == csum, "checksum")
    d["env_mask"] = d["env_mask"].reshape(n, env_words)
    _check((d["alias_servant"] < n).all(), "an alias names no servant")
    if mode & 2:
        ids = d["l_id"]
        _check((ids[1:] > ids[:-1]).all(), "lease ids not ascending")
        _check((ids < next_id).all(), "a lease id >= next_id")
        _check((d["l_state"] & LIVE != 0).all(), "a lease without the live bit")
        _check((d["l_servant"] < n).all(), "a lease names no servant")
        d["l_zombie"] = (d["l_state"] & ZOMBIE != 0).astype(np.uint8)
        d["l_stamp"] = d["l_state"] & np.uint32(STAMP)
    if mode & 4:
        rows = d["w_n_immediate"].astype(np.uint64) + d["w_n_prefetch"]
        _check((rows > 0).all() and int(rows.sum()) == n_rows, "rows(W) differs from the entries' sum")
    else:
        _check(n_rows == 0, "rows(W) without rpc mode")
    if mode & 8:
        _check((d["b_servant"] < n).all(), "a book entry names no servant")
    if mode & 16:
        _check((d["e_expires_at"] >= alive_bound).all(), "alive_bound above an expiry")
    return d


def build(d):
    """A blob from a dict shaped like parse()'s result. Lengths are taken from the columns; l_state may
    be left out (then l_zombie and, optionally, l_stamp make it); rep_tick, alive_bound, n_wait_rows,
    last_now, lease_tick and the alias columns have defaults. The result is checked with parse()."""
    mode = mode_of(d)
    env = np.ascontiguousarray(d["env_mask"], "<u8")
    n = len(d["version"])
    env = env.reshape(n, -1) if n else env.reshape(0, max(1, int(d.get("env_words", 1))))
    env_words = env.shape[1]
    cols = {k: v for k, v in d.items()}
    cols["env_mask"] = env.reshape(-1)
    cols.setdefault("rep_tick", np.zeros(n, np.uint32))
    cols.setdefault("alias_ip", np.empty(0, np.uint32))
    cols.setdefault("alias_servant", np.empty(0, np.uint32))
    n_l = len(cols["l_id"]) if mode & 2 else 0
    if mode & 2 and "l_state" not in cols:
        cols["l_state"] = (np.uint32(LIVE) | (np.asarray(cols["l_zombie"]).astype(np.uint32) << np.uint32(30)) |
                           np.asarray(cols.get("l_stamp", np.zeros(n_l, np.uint32)), np.uint32))
    n_w = len(cols["w_tag"]) if mode & 1 else 0
    n_b = len(cols["b_grant_id"]) if mode & 8 else 0
    n_alias = len(cols["alias_ip"])
    n_rows = int(d.get("n_wait_rows", (np.asarray(cols["w_n_immediate"], np.uint64) + cols["w_n_prefetch"]).sum()
                       if mode & 4 else 0))
    alive_bound = int(d.get("alive_bound", min([I64_MAX] + [int(x) for x in cols["e_expires_at"]]) if mode & 16
                            else I64_MAX))
    body, directory, off = [], [], HEADER_BYTES
    for name, sec, size in _sections(mode, env_words, n, n_alias, n_l, n_w, n_b):
        raw = b"".join(np.ascontiguousarray(cols[c], dt).tobytes() for c, dt, _ in sec)
        for c, dt, cnt in sec:
            if len(np.asarray(cols[c]).reshape(-1)) != cnt:
                raise FormatError("column %s has %d entries, %d expected" % (c, len(cols[c]), cnt))
        body.append(raw + bytes(size - len(raw)))
        directory += [off, size]
        off += size
    fields = [MAGIC, VERSION, HEADER_BYTES, off, 0, mode, env_words, n, n_alias] + [int(d.get(k, 0)) for k in CAPS] + [
        int(d.get("max_book", 0)), n_l, n_w, n_rows, n_b, int(d.get("lease_tick", 0)), int(d.get("next_id", 0)),
        int(d.get("last_now", I64_MIN)), alive_bound] + directory
    blob = bytearray(HEADER.pack(*fields) + b"".join(body))
    struct.pack_into("<Q", blob, 8 * CHECKSUM_WORD, checksum(blob))
    blob = bytes(blob)
    parse(blob)
    return blob


# ---- delta blobs (ydc_stream_delta / ydc_stream_delta_apply) ----
# The second, independent implementation of yadcc_amd/csrc/stream_delta_codec.h: a delta takes a leased,
# waiting-and-leased or rpc stream from the state of one full snapshot to that of a later one.
DELTA_MAGIC = 0x3141544C44434459  # "YDCDLTA1"
DELTA_VERSION = 1
DELTA_HEADER = struct.Struct("<QIIQQ4I4IQQq4IQqq8I14Q")
DELTA_HEADER_BYTES = 272
assert DELTA_HEADER.size == DELTA_HEADER_BYTES
DELTA_SECTIONS = ("inserted", "erased", "updated", "registry", "W", "E", "B")
# The registry's columns a heartbeat or a tick changes without a structural turn, in the blob's order.
DELTA_REGISTRY = ("version", "num_processors", "current_load", "servant_max_tasks", "flags", "running_tasks", "rep_tick")
_W_COLS = (("w_deadline", "<i8"), ("w_tag", "<u8"), ("w_lease_for", "<i8"), ("w_env_id", "<u4"), ("w_min_version", "<u4"),
           ("w_requestor_ip", "<u4"), ("w_n_immediate", "<u4"), ("w_n_prefetch", "<u4"))
_B_COLS = (("b_grant_id", "<u8"), ("b_servant_task_id", "<u8"), ("b_digest_key", "<u8"), ("b_servant", "<u4"))


def structure_stamp(d):
    """The stamp over what a delta does not carry, from a parsed full snapshot: mode bits, counts, the ten
    bounds and max_book (ten words, the fourth 0), every environment mask, then ip_id, alias ip and alias
    servant behind each other, zero-padded to a whole word; checksum() of that."""
    n, n_alias = len(d["version"]), len(d["alias_ip"])
    env = np.ascontiguousarray(d["env_mask"], "<u8").reshape(-1)
    env_words = int(d["env_words"])
    caps = [int(d[k]) for k in CAPS]
    head = [DELTA_MAGIC, mode_of(d) | env_words << 32, n | n_alias << 32, 0] + [
        caps[i] | caps[i + 1] << 32 for i in range(0, 10, 2)] + [int(d["max_book"])]
    tail = b"".join(np.ascontiguousarray(d[k], "<u4").tobytes() for k in ("ip_id", "alias_ip", "alias_servant"))
    tail += bytes(_pad8(len(tail)) - len(tail))
    return checksum(np.array(head, "<u8").tobytes() + env.tobytes() + tail)


def _delta_sections(mode, n, n_ins, n_era, n_upd, n_w, n_b, book_present):
    """[(name, [(column, dtype, count)], bytes)] in the blob's order."""
    rpc = mode & 4
    w = [(c, dt, n_w) for c, dt in _W_COLS if rpc or c not in ("w_n_immediate", "w_n_prefetch")] if mode & 1 else []
    secs = (("inserted", [("ins_id", "<u8", n_ins), ("ins_expires_at", "<i8", n_ins), ("ins_servant", "<u4", n_ins),
                          ("ins_state", "<u4", n_ins)]),
            ("erased", [("era_id", "<u8", n_era)]),
            ("updated", [("upd_id", "<u8", n_upd), ("upd_expires_at", "<i8", n_upd), ("upd_state", "<u4", n_upd)]),
            ("registry", [(k, "<u4", n) for k in DELTA_REGISTRY]),
            ("W", w),
            ("E", [("e_expires_at", "<i8", n)] if mode & 16 else []),
            ("B", [(c, dt, n_b) for c, dt in _B_COLS] if book_present else []))
    return [(name, cols, _pad8(sum(np.dtype(dt).itemsize * k for _, dt, k in cols))) for name, cols in secs]


_DELTA_FIELDS = ("mode", "env_words", "n_servants", "book_present", "max_leases", "max_waiting", "max_rows", "max_book",
                 "stamp", "base_next_id", "base_last_now", "base_lease_tick", "base_n_leases", "base_n_waiting", "reserved",
                 "next_id", "last_now", "alive_bound", "lease_tick", "n_leases", "n_waiting", "n_wait_rows", "n_book",
                 "n_ins", "n_era", "n_upd")


def parse_delta(blob):
    """The delta as a dict: the header's fields under _DELTA_FIELDS' names and every carried column. Raises
    FormatError for anything ydc_stream_delta_apply would refuse for its bytes alone."""
    blob = bytes(blob)
    _check(len(blob) >= DELTA_HEADER_BYTES, "shorter than a header")
    f = DELTA_HEADER.unpack_from(blob)
    magic, version, hbytes, total, csum = f[:5]
    d = dict(zip(_DELTA_FIELDS, f[5:31]))
    directory = f[31:45]
    _check(magic == DELTA_MAGIC, "not a stream delta (magic)")
    _check(version == DELTA_VERSION, "unknown format version")
    _check(hbytes == DELTA_HEADER_BYTES, "header size")
    _check(total == len(blob) and total % 8 == 0, "total bytes differ from the block's size")
    mode, n = d["mode"], d["n_servants"]
    _check(mode & ~31 == 0 and mode & 2, "mode bits")
    _check(not (mode & 4) or mode & 1, "rpc mode without W")
    _check(1 <= d["env_words"] <= 64, "env_words out of range")
    _check(d["book_present"] <= 1 and d["reserved"] == 0, "a reserved field is set")
    _check(not d["book_present"] or mode & 8, "B without the book")
    _check(d["max_leases"] > 0, "max_leases is 0")
    for bit, cap in ((1, d["max_waiting"]), (4, d["max_rows"]), (8, d["max_book"])):
        _check(bool(mode & bit) == bool(cap), "a bound does not fit the mode")
    _check(max(d["n_leases"], d["base_n_leases"]) <= d["max_leases"] and max(d["n_waiting"], d["base_n_waiting"]) <=
           d["max_waiting"] and d["n_book"] <= d["max_book"] and d["n_wait_rows"] <= d["max_rows"], "a count beyond its bound")
    _check(d["n_era"] + d["n_upd"] <= d["base_n_leases"], "more erased and updated leases than the base holds")
    _check(d["base_n_leases"] + d["n_ins"] - d["n_era"] == d["n_leases"], "|L| is not the base's + inserted - erased")
    _check(d["base_next_id"] <= d["next_id"] and d["n_ins"] <= d["next_id"] - d["base_next_id"],
           "more inserted leases than ids handed out")
    _check(d["last_now"] >= d["base_last_now"], "the clock runs backwards")
    for t in (d["lease_tick"], d["base_lease_tick"]):
        _check(t == 0 or t & STAMP, "a tick number whose stamp is 0")
    _check(mode & 16 or d["alive_bound"] == I64_MAX, "alive_bound without E")
    off = DELTA_HEADER_BYTES
    secs = _delta_sections(mode, n, d["n_ins"], d["n_era"], d["n_upd"], d["n_waiting"], d["n_book"], d["book_present"])
    for k, (name, cols, size) in enumerate(secs):
        _check(directory[2 * k] == off and directory[2 * k + 1] == size, "section %s is not where its counts put it" % name)
        _check(off + size <= len(blob), "section %s reaches past the end" % name)
        p = off
        for col, dt, cnt in cols:
            d[col] = np.frombuffer(blob, dt, cnt, p).copy()
            p += np.dtype(dt).itemsize * cnt
        _check(not any(blob[p:off + size]), "padding is not zero")
        off += size
    _check(off == len(blob), "bytes behind the last section")
    _check(checksum(blob) == csum, "checksum")
    for k in ("ins_id", "era_id", "upd_id"):
        _check((d[k][1:] > d[k][:-1]).all(), "%s not ascending" % k)
    _check(((d["ins_id"] >= d["base_next_id"]) & (d["ins_id"] < d["next_id"])).all(),
           "an inserted id outside [base next_id, next_id)")
    _check((d["era_id"] < d["base_next_id"]).all() and (d["upd_id"] < d["base_next_id"]).all(),
           "an erased or updated id >= the base's next_id")
    _check(not np.isin(d["era_id"], d["upd_id"]).any(), "a lease both erased and updated")
    _check((d["ins_state"] & LIVE != 0).all() and (d["upd_state"] & LIVE != 0).all(), "a carried lease without the live bit")
    _check((d["ins_servant"] < n).all(), "an inserted lease names no servant")
    if mode & 4:
        rows = d["w_n_immediate"].astype(np.uint64) + d["w_n_prefetch"]
        _check((rows > 0).all() and int(rows.sum()) == d["n_wait_rows"], "rows(W) differs from the entries' sum")
    else:
        _check(d["n_wait_rows"] == 0, "rows(W) without rpc mode")
    if d["book_present"]:
        _check((d["b_servant"] < n).all(), "a book entry names no servant")
    if mode & 16:
        _check((d["e_expires_at"] >= d["alive_bound"]).all(), "alive_bound above an expiry")
    return d


def build_delta(before, after):
    """The delta blob that takes the stream of the parsed full snapshot `before` to that of `after`: a
    function of the two snapshots alone. FormatError where there is none: another structure stamp, a
    stream without L, a lease on another servant."""
    _check(before.get("leased") and after.get("leased"), "a snapshot without L")
    st = structure_stamp(before)
    _check(st == structure_stamp(after), "the structure differs")
    mode, n = mode_of(after), len(after["version"])
    a_id, b_id = np.asarray(before["l_id"], np.uint64), np.asarray(after["l_id"], np.uint64)
    in_a, in_b = np.isin(b_id, a_id), np.isin(a_id, b_id)
    _check((b_id[~in_a] >= np.uint64(before["next_id"])).all(), "a lease appeared below the base's next_id")
    ka, kb = np.flatnonzero(in_b), np.flatnonzero(in_a)  # the leases in both, by position in each
    _check(np.array_equal(before["l_servant"][ka], after["l_servant"][kb]), "a lease changed its servant")
    ch = kb[(before["l_expires_at"][ka] != after["l_expires_at"][kb]) | (before["l_state"][ka] != after["l_state"][kb])]
    cols = dict(ins_id=b_id[~in_a], ins_expires_at=after["l_expires_at"][~in_a], ins_servant=after["l_servant"][~in_a],
                ins_state=after["l_state"][~in_a], era_id=a_id[~in_b], upd_id=b_id[ch],
                upd_expires_at=after["l_expires_at"][ch], upd_state=after["l_state"][ch])
    for k in DELTA_REGISTRY + tuple(c for c, _ in _W_COLS + _B_COLS) + ("e_expires_at",):
        if k in after:
            cols[k] = after[k]
    n_b = len(after["b_grant_id"]) if mode & 8 else 0
    book_present = int(bool(mode & 8) and (n_b != len(before["b_grant_id"]) or any(
        not np.array_equal(before[c], after[c]) for c, _ in _B_COLS)))
    n_w = len(after["w_tag"]) if mode & 1 else 0
    secs = _delta_sections(mode, n, len(cols["ins_id"]), len(cols["era_id"]), len(cols["upd_id"]), n_w, n_b, book_present)
    body, directory, off = [], [], DELTA_HEADER_BYTES
    for name, sec, size in secs:
        raw = b"".join(np.ascontiguousarray(cols[c], dt).tobytes() for c, dt, _ in sec)
        body.append(raw + bytes(size - len(raw)))
        directory += [off, size]
        off += size
    fields = [DELTA_MAGIC, DELTA_VERSION, DELTA_HEADER_BYTES, off, 0, mode, int(after["env_words"]), n, book_present,
              int(after["max_leases"]), int(after["max_waiting"]), int(after["max_rows"]), int(after["max_book"]), st,
              int(before["next_id"]), int(before["last_now"]), int(before["lease_tick"]), len(a_id),
              len(before["w_tag"]) if mode & 1 else 0, 0, int(after["next_id"]), int(after["last_now"]),
              int(after["alive_bound"]), int(after["lease_tick"]), len(b_id), n_w, int(after["n_wait_rows"]), n_b,
              len(cols["ins_id"]), len(cols["era_id"]), len(cols["upd_id"])] + directory
    blob = bytearray(DELTA_HEADER.pack(*fields) + b"".join(body))
    struct.pack_into("<Q", blob, 8 * CHECKSUM_WORD, checksum(blob))
    blob = bytes(blob)
    parse_delta(blob)
    return blob


def apply_delta(before, delta):
    """The parsed full snapshot that results when the delta (bytes or parse_delta's dict) is applied to the
    parsed full snapshot `before`: what ydc_stream_delta_apply makes of a standby in that state. FormatError
    where the delta's base is not `before`, an erased or updated id is missing, or an inserted one is there."""
    d = delta if isinstance(delta, dict) else parse_delta(delta)
    _check(before.get("leased") and d["mode"] == mode_of(before) and d["stamp"] == structure_stamp(before),
           "the delta's structure stamp is not this state's")
    ids = np.asarray(before["l_id"], np.uint64)
    _check((d["base_lease_tick"], d["base_next_id"], d["base_n_leases"], d["base_last_now"]) ==
           (before["lease_tick"], before["next_id"], len(ids), before["last_now"]) and
           d["base_n_waiting"] == (len(before["w_tag"]) if before.get("waiting") else 0), "the delta's base is not this state")
    _check(np.isin(d["era_id"], ids).all() and np.isin(d["upd_id"], ids).all(), "an erased or updated id is no lease")
    _check(not np.isin(d["ins_id"], ids).any(), "an inserted id is a lease already")
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    exp, state = out["l_expires_at"], out["l_state"]
    at = np.searchsorted(ids, d["upd_id"])
    exp[at], state[at] = d["upd_expires_at"], d["upd_state"]
    keep = ~np.isin(ids, d["era_id"])
    l_id = np.concatenate([ids[keep], d["ins_id"]])
    order = np.argsort(l_id, kind="stable")
    out["l_id"] = l_id[order]
    out["l_expires_at"] = np.concatenate([exp[keep], d["ins_expires_at"]])[order]
    out["l_servant"] = np.concatenate([out["l_servant"][keep], d["ins_servant"]])[order]
    out["l_state"] = np.concatenate([state[keep], d["ins_state"]])[order]
    out["l_zombie"] = (out["l_state"] & ZOMBIE != 0).astype(np.uint8)
    out["l_stamp"] = out["l_state"] & np.uint32(STAMP)
    for k in DELTA_REGISTRY + ("e_expires_at",) + tuple(c for c, _ in _W_COLS) + (
            tuple(c for c, _ in _B_COLS) if d["book_present"] else ()):
        if k in d:
            out[k] = d[k].copy()
    if not d["book_present"] and before.get("book"):
        _check(d["n_book"] == len(before["b_grant_id"]), "|B| differs without B")
    for k in ("next_id", "last_now", "lease_tick", "alive_bound", "n_wait_rows"):
        out[k] = d[k]
    return out


# ---- inspection sidecars (ydc_stream_delta_inspect / ydc_stream_inspect_restore /
# ydc_stream_delta_apply_inspected) ----
# The second, independent implementation of yadcc_amd/csrc/stream_inspect_delta_codec.h: what a full
# snapshot (kind 0) or a delta (kind 1) leaves out of a stream with inspection.
INSPECT_DELTA_MAGIC = 0x3144534E49434459  # "YDCINSD1"
INSPECT_DELTA_VERSION = 1
INSPECT_DELTA_HEADER = struct.Struct("<QIIQQ4IQQqIIQ4Q")
INSPECT_DELTA_HEADER_BYTES = 120
assert INSPECT_DELTA_HEADER.size == INSPECT_DELTA_HEADER_BYTES
INSPECT_FULL, INSPECT_DELTA = 0, 1
INSPECT_NO_ID, INSPECT_NO_TIME = 0xFFFFFFFF, I64_MIN
_INSPECT_FIELDS = ("kind", "n_servants", "n", "reserved", "stamp", "next_id", "last_now", "lease_tick", "n_leases", "epoch")
_INSPECT_IDENTITY = ("stamp", "next_id", "last_now", "lease_tick", "n_leases")
_INSPECT_RECORD = (("task_id", "<u8"), ("started_at", "<i8"), ("env_id", "<u4"), ("requestor_ip", "<u4"), ("prefetch", "u1"))
_INSPECT_SERVANT = (("discovered_at", "<i8"), ("ever_assigned", "<u8"))


def _inspect_sections(n, n_servants):
    secs = (("records", [(c, dt, n) for c, dt in _INSPECT_RECORD]), ("servants", [(c, dt, n_servants) for c, dt in _INSPECT_SERVANT]))
    return [(name, cols, _pad8(sum(np.dtype(dt).itemsize * k for _, dt, k in cols))) for name, cols in secs]


def parse_inspect_delta(blob):
    """The sidecar as a dict: the header's fields under _INSPECT_FIELDS' names, the records' columns under
    ydc_stream_inspect_tasks' names and the two servant columns. Raises FormatError for anything the
    three entry points would refuse for the bytes alone."""
    blob = bytes(blob)
    _check(len(blob) >= INSPECT_DELTA_HEADER_BYTES, "shorter than a header")
    f = INSPECT_DELTA_HEADER.unpack_from(blob)
    magic, version, hbytes, total, csum = f[:5]
    d = dict(zip(_INSPECT_FIELDS, f[5:15]))
    directory = f[15:19]
    _check(magic == INSPECT_DELTA_MAGIC, "not an inspection sidecar (magic)")
    _check(version == INSPECT_DELTA_VERSION, "unknown format version")
    _check(hbytes == INSPECT_DELTA_HEADER_BYTES, "header size")
    _check(total == len(blob) and total % 8 == 0, "total bytes differ from the block's size")
    _check(d["kind"] in (INSPECT_FULL, INSPECT_DELTA), "unknown kind")
    _check(d["reserved"] == 0, "a reserved field is set")
    _check(d["lease_tick"] == 0 or d["lease_tick"] & STAMP, "a tick number whose stamp is 0")
    _check(d["n"] <= d["n_leases"], "more records than leases")
    _check(d["kind"] != INSPECT_FULL or d["n"] == d["n_leases"], "a full sidecar whose records are not |L|")
    _check(d["n_leases"] <= d["next_id"], "more leases than ids handed out")
    off = INSPECT_DELTA_HEADER_BYTES
    for k, (name, cols, size) in enumerate(_inspect_sections(d["n"], d["n_servants"])):
        _check(directory[2 * k] == off and directory[2 * k + 1] == size, "section %s is not where its counts put it" % name)
        _check(off + size <= len(blob), "section %s reaches past the end" % name)
        p = off
        for col, dt, cnt in cols:
            d[col] = np.frombuffer(blob, dt, cnt, p).copy()
            p += np.dtype(dt).itemsize * cnt
        _check(not any(blob[p:off + size]), "padding is not zero")
        off += size
    _check(off == len(blob), "bytes behind the last section")
    _check(checksum(blob) == csum, "checksum")
    ids = d["task_id"]
    _check((ids[1:] > ids[:-1]).all(), "ids not ascending")
    _check((ids < np.uint64(d["next_id"])).all(), "an id >= next_id")
    _check((d["prefetch"] <= 1).all(), "a prefetch flag that is neither 0 nor 1")
    return d


def inspect_state(full, tasks, servants, epoch):
    """What build_inspect_delta is given: the identity of the parsed full snapshot `full`, the records of
    every lease (a dict shaped like binding.Context.stream_inspect_tasks' result), the two servant
    columns (... stream_inspect_servants') and the inspection epoch."""
    st = dict(stamp=structure_stamp(full), next_id=int(full["next_id"]), last_now=int(full["last_now"]),
              lease_tick=int(full["lease_tick"]), n_leases=len(full["l_id"]), epoch=int(epoch))
    for c, dt in _INSPECT_RECORD:
        st[c] = np.ascontiguousarray(tasks[c], dt)
    for c, dt in _INSPECT_SERVANT:
        st[c] = np.ascontiguousarray(servants[c], dt)
    _check(np.array_equal(st["task_id"], np.asarray(full["l_id"], np.uint64)), "the records are not L's")
    return st


def build_inspect_delta(state, ids, kind):
    """The sidecar of `kind` for the stream in `state` (inspect_state()): the records of the leases `ids`
    (ascending; ignored for INSPECT_FULL, which carries all of L) and the servant columns whole.
    FormatError where an id is no lease."""
    all_ids = state["task_id"]
    ids = all_ids if kind == INSPECT_FULL else np.asarray(ids, np.uint64).reshape(-1)
    at = np.searchsorted(all_ids, ids)
    _check(len(ids) == 0 or (at < len(all_ids)).all() and (all_ids[np.minimum(at, len(all_ids) - 1)] == ids).all(),
           "an id is no lease")
    cols = {c: state[c][at] for c, _ in _INSPECT_RECORD}
    cols.update({c: state[c] for c, _ in _INSPECT_SERVANT})
    n, n_servants = len(ids), len(state["discovered_at"])
    body, directory, off = [], [], INSPECT_DELTA_HEADER_BYTES
    for name, sec, size in _inspect_sections(n, n_servants):
        raw = b"".join(np.ascontiguousarray(cols[c], dt).tobytes() for c, dt, _ in sec)
        body.append(raw + bytes(size - len(raw)))
        directory += [off, size]
        off += size
    fields = [INSPECT_DELTA_MAGIC, INSPECT_DELTA_VERSION, INSPECT_DELTA_HEADER_BYTES, off, 0, int(kind), n_servants, n, 0,
              state["stamp"], state["next_id"], state["last_now"], state["lease_tick"], state["n_leases"],
              state["epoch"]] + directory
    blob = bytearray(INSPECT_DELTA_HEADER.pack(*fields) + b"".join(body))
    struct.pack_into("<Q", blob, 8 * CHECKSUM_WORD, checksum(blob))
    blob = bytes(blob)
    parse_inspect_delta(blob)
    return blob


def apply_inspect_delta(state, side, delta=None):
    """The inspect_state() that results. A full sidecar (ydc_stream_inspect_restore) is the state itself;
    `state` may be None. A delta sidecar (ydc_stream_delta_apply_inspected) needs its delta (bytes or
    parse_delta's dict): FormatError where the sidecar's identity is not the delta's result, its ids are
    not the delta's inserted ones, its epoch is not the state's, or the delta's base is not the state."""
    s = side if isinstance(side, dict) else parse_inspect_delta(side)
    out = {k: s[k] for k in _INSPECT_IDENTITY + ("epoch",)}
    for c, _ in _INSPECT_SERVANT:
        out[c] = s[c].copy()
    if s["kind"] == INSPECT_FULL:
        _check(delta is None, "a full sidecar beside a delta")
        for c, _ in _INSPECT_RECORD:
            out[c] = s[c].copy()
        return out
    _check(delta is not None, "a delta sidecar without its delta")
    d = delta if isinstance(delta, dict) else parse_delta(delta)
    _check(tuple(s[k] for k in _INSPECT_IDENTITY) == (d["stamp"], d["next_id"], d["last_now"], d["lease_tick"], d["n_leases"]),
           "the sidecar's identity is not the delta's result")
    _check(np.array_equal(s["task_id"], d["ins_id"]), "the sidecar's ids are not the delta's inserted ones")
    _check(s["epoch"] == state["epoch"], "the inspection epoch differs")
    _check((state["stamp"], state["next_id"], state["last_now"], state["lease_tick"], state["n_leases"]) ==
           (d["stamp"], d["base_next_id"], d["base_last_now"], d["base_lease_tick"], d["base_n_leases"]),
           "the delta's base is not this state")
    ids = state["task_id"]
    _check(np.isin(d["era_id"], ids).all() and not np.isin(d["ins_id"], ids).any(), "the delta's ids do not fit the state")
    _check(len(s["discovered_at"]) == len(state["discovered_at"]), "another number of servants")
    keep = ~np.isin(ids, d["era_id"])
    l_id = np.concatenate([ids[keep], s["task_id"]])
    order = np.argsort(l_id, kind="stable")
    out["task_id"] = l_id[order]
    for c, _ in _INSPECT_RECORD[1:]:
        out[c] = np.concatenate([state[c][keep], s[c]])[order]
    return out
