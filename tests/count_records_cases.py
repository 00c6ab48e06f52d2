"""The child process of tests/test_gpu_count_records.py: every case once through katome_dev_count_records under the switches of the
environment it was started with (they are read once per process), each compared as a whole sorted list with tests/count_model.py.

    python count_records_cases.py <repository root>

stdout: one JSON line per case -- what the case was and how the comparison ended; stderr: "CASE <name>" before a case's call, so
that the lines KATOME_LC_TRACE puts there can be told apart case by case.  A comparison that fails is reported and the next case
runs; a status that no case expects ends the process at once with status 3."""
import collections
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import count_model as cm                                    # noqa: E402
from katome_amd import _lib, device as kd                   # noqa: E402
from katome_amd.build import KatomePanic                    # noqa: E402

M64 = (1 << 64) - 1
SALT, SALT2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
MAX_RECORDS, MAX_OF_ONE_KEY = 2_500_000, 1 << 20          # the inputs' bounds: a group must never overfill a table
rng = np.random.default_rng(20261021)


def n_words(k):
    return 1 if 2 * k <= 62 else 2 if 2 * k <= 126 else 3


def random_keys(k, m):
    """up to m distinct keys of 2k bits, uniformly"""
    nw = n_words(k)
    words = rng.integers(0, 1 << 64, size=(m, nw), dtype=np.uint64)
    mask = (1 << (2 * k)) - 1
    keys = {(sum(int(w) << (64 * (nw - 1 - i)) for i, w in enumerate(row))) & mask for row in words.tolist()}
    return sorted(keys)


def one_orientation(keys, k, taken=()):
    """of every k-mer among the keys one orientation only, none that `taken` (keys with their reverse complements) holds already"""
    seen, out = set(taken), []
    for key in keys:
        other = cm.revcomp(key, k)
        if key in seen or other in seen:
            continue
        seen.add(key); seen.add(other)
        out.append(key)
    return out


def palindromes(k, m):
    """m distinct k-mers of even k that are their own reverse complement: a half and its reverse complement behind it"""
    h = k // 2
    out = []
    for half in random_keys(h, m)[:m] if 4 ** h > m else range(4 ** h):
        out.append((half << (2 * h)) | cm.revcomp(half, h))
    assert all(cm.revcomp(p, k) == p for p in out)
    return out[:m]


def filler(k, n, rc, avoid=()):
    """about n records: random keys repeated 1 to 9 times each, weights 1"""
    taken = set(avoid) | ({cm.revcomp(a, k) for a in avoid} if rc else set())
    keys = random_keys(k, max(n // 5, 1))
    keys = one_orientation(keys, k, taken) if rc else [x for x in keys if x not in taken]
    if 4 ** k <= 64:                        # (k = 3: every key there is, the records spread over them)
        reps = np.full(len(keys), max(n // max(len(keys), 1), 1))
    else:
        reps = rng.integers(1, 10, len(keys))
    recs = [key for key, r in zip(keys, reps.tolist()) for _ in range(r)]
    return recs, [1] * len(recs)


def split_sum(total):
    """records whose weights add up to `total` (up to 2^33): as few as u32 allows, in two ways where there are two"""
    ways = []
    if total <= cm.M32:
        ways.append([total])
    if total >= 2:
        a = min(total // 2, cm.M32)
        rest = total - a
        ways.append([a, rest] if rest <= cm.M32 else [a, cm.M32, rest - cm.M32])
    return ways


CASES = []


def case(name, k, rc, min_weight, recs, wts, n_parts=0, unit=False, expect="OK", huge=False):
    CASES.append(dict(name=name, k=k, rc=rc, min_weight=min_weight, recs=recs, wts=None if unit else wts, n_parts=n_parts, expect=expect, huge=huge))


def with_filler(name, k, rc, min_weight, special, n=20000, **kw):
    """`special`: [(key, [weights of its records])] among about n records of filler"""
    recs, wts = filler(k, n, rc, [key for key, _ in special])
    for key, ws in special:
        recs += [key] * len(ws); wts += ws
    case(name, k, rc, min_weight, recs, wts, **kw)


ONE, TWO, THREE = (3, 16, 31), (32, 40, 63), (64, 95)

# uniform random keys, each 1 to 9 times, weights 1; both strands with a threshold, even k with self-complementary k-mers among them
for k in (16, 31, 32, 40, 63, 64, 95):
    n = 20000 if n_words(k) == 1 else 70000             # (two and three words: enough for the default route to sample the level)
    case("uniform_k%d" % k, k, False, 0, *filler(k, n, False))
    if n_words(k) < 3:
        pal = palindromes(k, 60) if k % 2 == 0 else []
        recs, wts = filler(k, n, True, pal)
        for i, p in enumerate(pal):
            recs += [p] * (1 + i % 4); wts += [1] * (1 + i % 4)
        case("uniform_rc_k%d_t3" % k, k, True, 3, recs, wts)
# all 64 keys of k = 3 in 100 000 records
case("all64_k3", 3, False, 0, *filler(3, 100000, False))
case("all64_rc_k3_t2", 3, True, 2, *filler(3, 100000, True))

# a weight ladder: every weight on a key of its own
LADDER = (0, 1, 0xFFFE, 0xFFFF, 0x10000, 1 << 31, cm.M32)
for k in (16, 31, 40, 63, 64):
    for rc, t in ((False, 0), (True, 1)):
        if rc and n_words(k) == 3:
            continue
        keys = one_orientation(random_keys(k, 40), k)[:len(LADDER)]
        with_filler("ladder%s_k%d_t%d" % ("_rc" if rc else "", k, t), k, rc, t, [(key, [w]) for key, w in zip(keys, LADDER)])

# sums at the 16-bit and the 32-bit edge.  fit: nothing beyond 16 bits, a sum of exactly 0xFFFF among them (the 8-byte slots keep the
# level); carry: every record within 16 bits, one sum one beyond (those slots must give up); wrap: the sums of the issue's list
for k in (16, 31, 40, 64):
    rc = k == 31
    keys = one_orientation(random_keys(k, 60), k)
    with_filler("sums_fit_k%d" % k, k, rc, 0, [(keys[0], [0x7FFF, 0x7FFF, 1]), (keys[1], [0xFFFF]), (keys[2], [0xFFFE, 1]), (keys[3], [1] * 300)])
    with_filler("sums_carry_k%d" % k, k, rc, 0, [(keys[0], [0x7FFF, 0x7FFF, 1]), (keys[1], [0xFFFF, 1]), (keys[2], [0x8000, 0x8000])])
    special = []
    for i, total in enumerate((0xFFFF, 0x10000, cm.M32, 1 << 32, (1 << 32) + 5)):
        for j, ws in enumerate(split_sum(total)):
            special.append((keys[10 + 2 * i + j], ws))
    special.append((keys[30], [1 << 31, 1 << 31, 5]))
    special.append((keys[31], [cm.M32, 6]))
    with_filler("sums_wrap_k%d" % k, k, rc, 0, special)
    if n_words(k) < 3:               # (three words: never thresholded)
        with_filler("sums_wrap_k%d_t1" % k, k, rc, 1, special)          # (the sum that wraps to 0 goes at threshold 1)

# the threshold at its boundary
for k in (16, 31, 40, 63):
    for rc in (False, True):
        for t in (1, 2, 7, 0x10000, cm.M32):
            keys = one_orientation(random_keys(k, 80), k)
            special, i = [], 0
            for total in (t - 1, t, t + 1):
                for ws in split_sum(total):
                    special.append((keys[i], ws)); i += 1
            if rc and k % 2 == 0:        # self-complementary: twice the sum meets the threshold, in 32 bits
                for total, p in zip(sorted({max(t // 2 - 1, 0), t // 2, (t + 1) // 2, 1 << 31, (1 << 31) + (t + 1) // 2}), palindromes(k, 12)):
                    for j, ws in enumerate(split_sum(total)[-1:]):
                        special.append((p, ws))
            with_filler("threshold%s_k%d_t%x" % ("_rc" if rc else "", k, t), k, rc, t, special)

# key extremes, one strand: 0, 4^k - 1, their single-bit neighbours at both ends, and the reverse complements of all of them
for k in ONE + TWO + THREE:
    top = 4 ** k - 1
    keys = {0, top, 1, top ^ 1, 1 << (2 * k - 1), top ^ (1 << (2 * k - 1)), 2, top ^ 2, 1 << (2 * k - 2), top ^ (1 << (2 * k - 2))}
    if n_words(k) > 1:                   # ... and at the seams of the words
        keys |= {1 << 63, 1 << 64, top ^ (1 << 63), top ^ (1 << 64), M64, M64 + 1}
    keys = {x for x in keys if x <= top}
    keys |= {cm.revcomp(x, k) for x in keys}
    with_filler("extremes_k%d" % k, k, False, 0, [(key, [1 + i % 3] * (1 + i % 4)) for i, key in enumerate(sorted(keys))])

# the salt that marks "not set" in the whole-key slots as a key's second or third word
for k, rc in ((32, False), (40, False), (40, True), (63, False), (63, True)):
    mask_hi = (1 << (2 * k - 64)) - 1
    keys = one_orientation([SALT] + [((int(h) & mask_hi) << 64) | SALT for h in rng.integers(0, 1 << 62, 6)], k)
    with_filler("salt%s_k%d" % ("_rc" if rc else "", k), k, rc, 2 if rc else 0, [(key, [3, 4]) for key in keys], n=70000)
for k in THREE:
    mask_hi = (1 << (2 * k - 128)) - 1
    r = [int(x) for x in rng.integers(0, 1 << 62, 12)]
    second = [((r[i] & mask_hi) << 128) | (SALT << 64) | r[i + 1] for i in range(0, 4, 2)] + [SALT << 64, (SALT << 64) | SALT]
    third = [((r[i] & mask_hi) << 128) | (r[i + 1] << 64) | SALT for i in range(4, 8, 2)] + [SALT]
    third2 = [((r[i] & mask_hi) << 128) | (r[i + 1] << 64) | SALT2 for i in range(8, 12, 2)] + [SALT2]
    with_filler("salt_second_k%d" % k, k, False, 0, [(key, [3, 4]) for key in second], n=70000)
    with_filler("salt_third_k%d" % k, k, False, 0, [(key, [3, 4]) for key in third], n=70000)
    with_filler("salt_third_own_k%d" % k, k, False, 0, [(key, [3, 4]) for key in third2], n=70000)

# no weights array: every record counts once (two and three words)
for k in TWO + THREE:
    case("unit_k%d" % k, k, False, 0, *filler(k, 70000, False), unit=True)
for k in (40, 63):
    case("unit_rc_k%d_t2" % k, k, True, 2, *filler(k, 70000, True), unit=True)

# one group beyond the 20 bits of the fingerprint slots' representative
recs, wts = filler(40, 50000, False)
HUGE_KEY = random_keys(40, 1)[0]
case("huge_group_k40", 40, False, 0, recs + [HUGE_KEY] * ((1 << 20) + 1), wts + [1] * ((1 << 20) + 1), huge=True)

# nothing and one record
for k in (16, 40, 64):
    case("n0_k%d" % k, k, False, 0, [], [])
    case("n1_k%d" % k, k, False, 0, [random_keys(k, 1)[0]], [cm.M32])
case("n1_rc_k16", 16, True, 0, [palindromes(16, 1)[0]], [(1 << 31) + 1])

# the owner split: k = 31, one strand
recs, wts = filler(31, 20000, False)
wts = [int(w) for w in rng.choice(np.array([0, 1, 2, 0xFFFF, 0x10000, cm.M32], np.uint64), len(recs))]
for parts in (1, 2, 3, 8, 16):
    case("owners_%d" % parts, 31, False, 0, recs, wts, n_parts=parts)
case("owners_17_refused", 31, False, 0, recs, wts, n_parts=17, expect="E_ARG")
case("owners_rc_refused", 31, True, 0, recs, wts, n_parts=2, expect="E_ARG")
case("owners_threshold_refused", 31, False, 1, recs, wts, n_parts=2, expect="E_ARG")
case("owners_two_words_refused", 40, False, 0, *filler(40, 20000, False), n_parts=2, expect="E_ARG")
# what else the count itself refuses
case("unit_one_word_refused", 31, False, 0, recs, wts, unit=True, expect="E_ARG")
case("three_words_rc_refused", 64, True, 0, *filler(64, 20000, False), expect="E_UNSUPPORTED")
case("three_words_threshold_refused", 64, False, 1, *filler(64, 20000, False), expect="E_UNSUPPORTED")


def to_device(recs, wts, k):
    nw = n_words(k)
    if nw == 1:
        host = np.array(recs, np.uint64).reshape(-1)
    else:
        host = np.array([[(x >> (64 * (nw - 1 - i))) & M64 for i in range(nw)] for x in recs], np.uint64).reshape(-1)
    keys = torch.from_numpy(host.view(np.int64).copy()).cuda()
    weights = None if wts is None else torch.from_numpy(np.array(wts, np.uint64).astype(np.uint32).view(np.int32).copy()).cuda()
    return keys, weights


def from_device(keys, weights, nw):
    rows = keys.cpu().numpy().view(np.uint64).reshape(-1, nw).tolist()
    ints = [row[0] for row in rows] if nw == 1 else [sum(w << (64 * (nw - 1 - i)) for i, w in enumerate(row)) for row in rows]
    return list(zip(ints, weights.cpu().numpy().view(np.uint32).tolist()))


def first_difference(got, want):
    if len(got) != len(want):
        head = "%d entries for %d" % (len(got), len(want))
    else:
        head = "same length"
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "%s; entry %d: got (%x, %d), the model has (%x, %d)" % (head, i, g[0], g[1], w[0], w[1])
    return head


def run(c):
    k, rc, t, parts = c["k"], c["rc"], c["min_weight"], c["n_parts"]
    order = rng.permutation(len(c["recs"])).tolist()
    recs = [c["recs"][i] for i in order]
    wts = None if c["wts"] is None else [c["wts"][i] for i in order]
    nw, n = n_words(k), len(recs)
    # the condition on the inputs: no key of more than 2^20 records -- but for the one case that is about that --, no level beyond 2.5 M
    times = collections.Counter(recs)
    true_sums = dict(times)                          # (what a key's records add up to before anything wraps)
    if wts is not None and any(w != 1 for w in wts):
        true_sums = {}
        for key, w in zip(recs, wts):
            true_sums[key] = true_sums.get(key, 0) + w
    assert n <= MAX_RECORDS and all(0 <= key < 4 ** k for key in times), c["name"]
    assert c["huge"] == (max(times.values(), default=0) > MAX_OF_ONE_KEY), c["name"]
    row = dict(name=c["name"], k=k, nw=nw, rc=rc, min_weight=t, n=n, n_parts=parts, weights=wts is not None, huge=c["huge"], expect=c["expect"],
               over16=wts is not None and (any(w == 0 or w > 0xFFFF for w in wts) or any(s > 0xFFFF for s in true_sums.values())),
               salt=nw > 1 and any(((key >> (64 * (nw - 2))) & M64) == SALT or (nw == 3 and (key & M64) == SALT2) for key in times))
    keys_d, weights_d = to_device(recs, wts, k)
    sys.stderr.write("CASE %s\n" % c["name"]); sys.stderr.flush()
    try:
        out_k, out_w, n_out, distinct, base, count = kd.count_records(keys_d, weights_d, k, rc, t, parts)
        row["status"] = "OK"
    except KatomePanic as e:
        row["status"], row["message"] = e.name, e.message
        if e.name not in ("E_UNSUPPORTED", "E_ARG") or (e.name != c["expect"] and not c["huge"]):
            print(json.dumps(row)); sys.stdout.flush()
            sys.exit(3)
    if row["status"] != "OK" and not c["huge"]:
        row["ok"] = row["status"] == c["expect"]
        return row
    if c["expect"] != "OK":
        row["ok"], row["detail"] = False, "not refused"
        return row
    want = cm.count(recs, wts, k, rc, t)
    if row["status"] != "OK":
        # the group beyond 20 bits, refused: the same records counted in the hash table, as a build does then
        b = kd.Builder(k, rc)
        b.insert(keys_d, weights_d)
        dg = b.finalize()
        got = sorted(from_device(dg.edge_key.reshape(-1), dg.edge_weight, nw))
        row["ok"], row["route"] = got == want and dg.n_edges == len(want), "table"
        if not row["ok"]:
            row["detail"] = first_difference(got, want)
        del dg
        b.close()
        return row
    got = from_device(out_k, out_w, nw)
    if not parts:
        got.sort()
        ok = got == want and n_out == len(want) and distinct == cm.n_distinct(recs)
        detail = "" if got == want else first_difference(got, want)
        if not ok:
            detail += "; n_out %d for %d, n_distinct %d for %d" % (n_out, len(want), distinct, cm.n_distinct(recs))
    else:
        # owner p's stretch holds exactly the model's keys of that owner with their sums; the stretches do not overlap
        owner = dict(zip([key for key, _ in want], cm.owners([key for key, _ in want], k, parts)))
        ok, detail, end = n_out == len(want) == sum(count) and distinct == len(want), "", 0
        for p, (b0, cnt) in sorted(enumerate(zip(base, count)), key=lambda x: x[1][0]):
            if cnt and b0 < end:
                ok, detail = False, detail + "owner %d's stretch begins inside another; " % p
            if b0 + cnt > n:
                ok, detail = False, detail + "owner %d's stretch ends beyond the records; " % p
                continue
            end = max(end, b0 + cnt)
            mine, theirs = sorted(got[b0:b0 + cnt]), [e for e in want if owner[e[0]] == p]
            if mine != theirs:
                ok, detail = False, detail + "owner %d: %s; " % (p, first_difference(mine, theirs))
        row["owners_used"] = sum(1 for cnt in count if cnt)
    row["ok"], row["n_out"], row["n_distinct"] = ok, n_out, distinct
    if not ok:
        row["detail"] = detail
    return row


def arguments():
    """what the entry itself refuses, on the raw prototype"""
    L = _lib.lib()
    keys = torch.zeros(8, dtype=torch.int64, device="cuda")
    wts = torch.ones(8, dtype=torch.int32, device="cuda")
    out_k, out_w = torch.zeros(64, dtype=torch.int64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    a, b = C.c_uint64(), C.c_uint64()
    own = (C.c_uint64 * 16)()
    P = kd._ptr

    def call(d_keys=keys, n=8, k=31, rc=0, n_parts=0, d_out=out_k, cap=9, n_out=C.byref(a), base=None):
        return _lib.STATUS.get(L.katome_dev_count_records(0, P(d_keys), P(wts), n, k, rc, 0, n_parts, P(d_out), P(out_w), cap, n_out, C.byref(b), base, base, None))
    got = dict(fine=call(), null_keys=call(d_keys=None), null_out=call(d_out=None), null_n_out=call(n_out=None), k1=call(k=1), k96=call(k=96),
               capacity=call(cap=8), capacity_rc=call(rc=1, cap=16), capacity_rc_fine=call(rc=1, cap=17), owners_without_arrays=call(n_parts=2),
               owners_17=call(n_parts=17, base=own), nothing=call(d_keys=None, d_out=None, n=0, cap=1))
    want = dict(fine="OK", null_keys="E_ARG", null_out="E_ARG", null_n_out="E_ARG", k1="E_ARG", k96="E_ARG", capacity="E_ARG", capacity_rc="E_ARG",
                capacity_rc_fine="OK", owners_without_arrays="E_ARG", owners_17="E_ARG", nothing="OK")
    return dict(name="arguments", ok=got == want, status="OK", expect="OK", n=0, got=got)


if __name__ == "__main__":
    for c in CASES:
        print(json.dumps(run(c))); sys.stdout.flush()
    sys.stderr.write("CASE arguments\n"); sys.stderr.flush()
    print(json.dumps(arguments())); sys.stdout.flush()
    torch.cuda.synchronize()
