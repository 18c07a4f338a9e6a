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
