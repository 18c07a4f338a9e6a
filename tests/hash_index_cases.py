"""Keys of one home slot for the three open-addressing tables of an open stream that hash with
splitmix64's finaliser: the digest index over the book (yadcc_amd/csrc/book_index.h), the load per
requestor (requestor_index.h) and the tick's quota table (stream_quota.h). The arithmetic they share
(index_home.h) is restated here in plain Python integers with its own copy of the constants:

  home(key) = mix(key) & (slots - 1), then linear probing;
  slots     = the smallest power of two >= 2 n, never fewer than 1024 (n: |B|, |L| + |W|, max_tasks).

tests/test_hash_index_model.py pins the restatement (on the CPU, and against the library's own header
through tests/native/hash_home_test.cc); tests/test_hash_index_gpu.py feeds the keys to the kernels.

mix is a bijection on 64 bits: an xor with a right shift is undone by iterating it, an odd multiplier
has an inverse modulo 2^64. A digest key of home h at `bits` is therefore unmix((r << bits) | h) for
any r, and bit `bits` of the mix, the lowest bit of r, says where the key goes when the table doubles:
keys that share it stay one chain, keys that differ in it split into chains at h and h + 2^bits. A
requestor id has 32 bits only, so ids of one home are FOUND, by a NumPy sweep over consecutive ids.

What the GPU tests may rest on, and nothing more: the SET of occupied slots does not depend on the
order of the inserts; n keys of one home occupy n consecutive slots from it; the largest displacement
is n - 1 in every order. Which key sits in which slot is the business of whoever won the CAS.
"""
import numpy as np

M64 = (1 << 64) - 1
ALL = M64              # the book index's free-slot mark: an ordinary key with a side record, never on a chain
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
C1_INV, C2_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)
assert (C1 * C1_INV) & M64 == 1 and (C2 * C2_INV) & M64 == 1
FLOOR = 1024           # no table has fewer slots
FLOOR_BITS = 10
HOMES = (100, 1021, 1023)   # mid-table; the run crosses the wrap; only the first member stays in the last slot
LENGTHS = (1, 2, 63, 64, 65, 257)
STEP = 0x2545F4914F6CDD1D   # odd: r walks its whole range


def mix(x):
    """book_index_mix: splitmix64's finaliser."""
    x &= M64
    x ^= x >> 30
    x = (x * C1) & M64
    x ^= x >> 27
    x = (x * C2) & M64
    x ^= x >> 31
    return x


def _unshift(y, s):
    """The x with x ^ (x >> s) == y: every round fixes s more bits from the top."""
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def unmix(y):
    y &= M64
    x = _unshift(y, 31)
    x = (x * C2_INV) & M64
    x = _unshift(x, 27)
    x = (x * C1_INV) & M64
    return _unshift(x, 30)


def mix_np(x):
    """mix on a uint64 array (the products wrap modulo 2^64)."""
    x = np.asarray(x, np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(C1)
    x ^= x >> np.uint64(27)
    x *= np.uint64(C2)
    x ^= x >> np.uint64(31)
    return x


def home(key, bits):
    return mix(key) & ((1 << bits) - 1)


def _slots(n, most=None):
    s = FLOOR
    while s < 2 * n and (most is None or s < most):
        s <<= 1
    return s


def slots_book(n):
    """book_index_slots: n entries of B (n <= 2^30)."""
    return _slots(n)


def slots_requestor(n):
    """requestor_index_slots: n entries of L and W together."""
    return _slots(n, 1 << 31)


def slots_quota(max_tasks):
    """quota_slots: a stream with max_tasks new requests per tick."""
    return _slots(max_tasks, 1 << 31)


def slots_usage(n):
    """usage_slots: n distinct requestors of the usage table (stream_usage.h)."""
    return _slots(n, 1 << 31)


def bits_of(slots):
    assert slots >= FLOOR and slots & (slots - 1) == 0
    return slots.bit_length() - 1


def _kind_bit(kind, k):
    """Bit `bits` of the mix of the k-th collider. "stay0" / "stay1": all alike; "split": in turns."""
    return {"stay0": 0, "stay1": 1, "split": k & 1}[kind]


def key_colliders(bits, h, n, kind="any", zero=False):
    """n distinct 64-bit keys with home(key, bits) == h, in the order they are made (scattered, not
    sorted). kind: "any", or "stay0" / "stay1" / "split" (_kind_bit). Never all ones; 0 (whose home is 0)
    only with zero=True, and then first."""
    assert 0 <= h < (1 << bits) and kind in ("any", "stay0", "stay1", "split")
    out, seen = [], set()
    if zero:
        assert h == 0 and kind in ("any", "stay0", "split"), "mix(0) == 0: key 0 lives at home 0"
        out.append(0)
        seen.add(0)
    top = (1 << (64 - bits)) - 1
    r = 1
    while len(out) < n:
        r = (r + STEP) & top
        q = r
        if kind != "any":
            q = (r & ~1) | _kind_bit(kind, len(out))
        key = unmix((q << bits) | h)
        if key in seen or key == ALL or key == 0:
            continue
        seen.add(key)
        out.append(key)
    return out[:n]


def ip_colliders(bits, h, n, lo=0x0A000000, kind="any", skip=()):
    """n distinct 32-bit ids with home(id, bits) == h, ascending from `lo`, none of `skip`: a sweep over
    consecutive ids (about one in 2^bits has the home). kind as key_colliders'."""
    assert 0 <= h < (1 << bits) and kind in ("any", "stay0", "stay1", "split")
    out, skip, at = [], set(int(s) for s in skip), lo
    mask, nxt = np.uint64((1 << bits) - 1), np.uint64(bits)
    while len(out) < n:
        assert at < (1 << 32), "the sweep ran out of 32-bit ids"
        ids = np.arange(at, min(at + (1 << 20), 1 << 32), dtype=np.uint64)
        m = mix_np(ids)
        hit = (m & mask) == np.uint64(h)
        for ip, b in zip(ids[hit].tolist(), ((m[hit] >> nxt) & np.uint64(1)).tolist()):
            if len(out) == n:
                break
            if ip in skip or (kind != "any" and b != _kind_bit(kind, len(out))):
                continue
            out.append(ip)
        at += 1 << 20
    return out


def probe(keys, bits):
    """The inserts of `keys` in the given order (a key that is in the table already is found, not
    inserted): [(key, slot, displacement)]. The slots of single keys depend on the order; see layout()."""
    mask = (1 << bits) - 1
    taken, out = {}, []
    for key in keys:
        h, d = home(key, bits), 0
        while (h + d) & mask in taken and taken[(h + d) & mask] != key:
            d += 1
        if (h + d) & mask not in taken:
            taken[(h + d) & mask] = key
            out.append((key, (h + d) & mask, d))
    return out


def layout(keys, bits):
    """-> (the set of occupied slots, the largest displacement) after inserting `keys` in the order given."""
    p = probe(keys, bits)
    return frozenset(s for _, s, _ in p), max([d for _, _, d in p] + [0])


def run_of(h, n, bits):
    """The n consecutive slots from h."""
    return frozenset((h + d) & ((1 << bits) - 1) for d in range(n))


def one_chain(keys, bits, h):
    """Asserts that `keys` are distinct keys of home h at `bits` that form one run from it, in any
    order; -> the run. What every case asserts of its keys before it plays them."""
    keys = [int(k) for k in keys]
    n = len(keys)
    assert len(set(keys)) == n and all(home(k, bits) == h for k in keys), "not %d distinct keys of home %d" % (n, h)
    occ, md = layout(keys, bits)
    assert occ == run_of(h, n, bits) and md == n - 1, (h, n, md)
    assert layout(keys[::-1], bits) == (occ, md)
    return occ


def histogram(keys, bits):
    """Displacement -> number of inserts; "wrap": the inserts whose probe went from the last slot to slot 0."""
    hist = {}
    for key, slot, d in probe(keys, bits):
        hist[d] = hist.get(d, 0) + 1
        if slot < home(key, bits):
            hist["wrap"] = hist.get("wrap", 0) + 1
    return hist


def absent_around(bits, h, n, members, same=16, ids=False):
    """Keys that are NOT in a table holding the chain `members` (n keys of home h) and whose probes meet
    its run: `same` of home h (they walk the whole run before they may answer "absent"), one of home
    h + 1 and one of h + n - 1 (inside the run), one of h + n (the first free slot). ids: 32-bit ids."""
    mask = (1 << bits) - 1
    make = (lambda hh, k, skip: ip_colliders(bits, hh, k, skip=skip)) if ids else (
        lambda hh, k, skip: [x for x in key_colliders(bits, hh, k + len(skip)) if x not in skip][:k])
    members = set(int(m) for m in members)
    out = make(h, same, members)
    for hh in sorted({(h + 1) & mask, (h + n - 1) & mask, (h + n) & mask} - {h}):
        out += make(hh, 1, members)
    assert not members & set(out)
    return out
