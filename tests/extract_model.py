"""The extraction entries restated on strings (include/katome_gpu.h and kmer_bits.h's header have the formats):
    window        `length` bases of a read from base `start`; its value is the base-4 number A=0 C=1 G=2 T=3, first base on top
    canonical     with rc, the smaller of the window and its reverse complement; "flipped" iff the complement is strictly smaller
    record        that value right-aligned in nw 64-bit words, most significant word first; nw = 1 up to 31 bases, 2 up to 63, 3 up to 95
    mark          first-seen builders with rc: bit 62 of word 0 of a flipped record (above every base bit at each nw)
    skipped read  every record of it is all ones
    tile          record j of a read is the (k+span-1)-mer at window j*span, (L-k+1)//span of them; the remainder is the plain
                  windows from ((L-k+1)//span)*span on
What tests/test_gpu_extract.py compares extract.hip with, record for record.  Strings, Python integers and numpy only: nothing here
comes from kmer_bits.h, the host shim or the library's own helpers."""
import numpy as np

from helpers import pack_reads_ascii, revcomp_str

MARK_BIT = 62
_TO4 = str.maketrans("ACGT", "0123")
_ASCII = np.frombuffer(b"ACGT", np.uint8)


def words_for(bases):
    return 1 if bases <= 31 else 2 if bases <= 63 else 3


def kmer_value(s):
    """helpers.kmer_to_int, quicker (test_extract_model_host pins the two equal)"""
    return int(s.translate(_TO4), 4)


def window_record(seq, start, length, rc, mark=False):
    """-> (value, marked): the window's 2*length-bit integer (canonical with rc), and whether a marking builder tags it.  The mark is
    never part of the integer: which bit it lands in depends on the words the record is formatted into (format_words)"""
    s = seq[start:start + length]
    assert len(s) == length
    v = kmer_value(s)
    if not rc:
        return v, False
    r = kmer_value(revcomp_str(s))
    return (r, bool(mark)) if r < v else (v, False)


def format_words(values, marked, nw):
    """Python integers (None: a skipped read's record) -> [n, nw] uint64, most significant word first; bit 62 of word 0 where marked"""
    ones = (1 << (64 * nw)) - 1
    buf = b"".join((ones if v is None else v).to_bytes(8 * nw, "big") for v in values)
    out = np.frombuffer(buf, dtype=">u8").astype(np.uint64).reshape(-1, nw)
    m = np.asarray(marked, dtype=bool)
    if m.any():
        out[m, 0] |= np.uint64(1 << MARK_BIT)
    return out


def _rows(reads):
    return [bytes(row).decode() for row in np.asarray(reads, dtype=np.uint8)]


def _stepped(reads, first, step, count, length, rc, skip, mark):
    """`count` records per read: windows of `length` bases at first, first + step, ..."""
    values, marked = [], []
    for r, s in enumerate(_rows(reads)):
        for j in range(count):
            if skip is not None and skip[r]:
                v, m = None, False
            else:
                v, m = window_record(s, first + j * step, length, rc, mark)
            values.append(v)
            marked.append(m)
    return format_words(values, marked, words_for(length))


# ---- the same, whole columns at a time (the cases of hundreds of thousands of reads); pinned equal to the above ------------------
def _np_words(win):
    """codes [m, length] -> [m, nw] uint64, most significant word first"""
    m, length = win.shape
    nw = words_for(length)
    out = np.zeros((m, nw), np.uint64)
    for i in range(length):
        pos = 2 * (length - 1 - i)
        out[:, nw - 1 - pos // 64] |= win[:, i].astype(np.uint64) << np.uint64(pos % 64)
    return out


def _np_stepped(reads, first, step, count, length, rc, skip, mark):
    reads = np.asarray(reads, dtype=np.uint8)
    codes = np.zeros(256, np.uint8)
    codes[_ASCII] = np.arange(4, dtype=np.uint8)
    codes = codes[reads]
    n, nw = reads.shape[0], words_for(length)
    out = np.empty((n, count, nw), np.uint64)
    for j in range(count):
        win = codes[:, first + j * step:first + j * step + length]
        assert win.shape[1] == length
        f = _np_words(win)
        if rc:
            c = _np_words(3 - win[:, ::-1])
            lt, eq = np.zeros(n, bool), np.ones(n, bool)
            for w in range(nw):
                lt |= eq & (c[:, w] < f[:, w])
                eq &= c[:, w] == f[:, w]
            f[lt] = c[lt]
            if mark:
                f[lt, 0] |= np.uint64(1 << MARK_BIT)
        out[:, j] = f
    if skip is not None:
        out[np.asarray(skip, dtype=bool)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return out.reshape(n * count, nw)


def _fixed(reads, first, step, count, length, rc, skip, mark, fast):
    return (_np_stepped if fast else _stepped)(reads, first, step, count, length, rc, skip, mark)


def with_skipped(records, skip):
    """records of reads of one length, none skipped -> the same with every record of a skipped read all ones"""
    out = records.copy()
    if out.size:
        out.reshape(len(skip), -1)[np.asarray(skip, dtype=bool)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return out


# ---- reads of one length: `reads` is [n, L] ASCII -----------------------------------------------------------------------------------
def fixed_records(reads, k, rc, skip=None, mark=False, fast=False):
    L = np.asarray(reads).shape[1]
    return _fixed(reads, 0, 1, L - k + 1, k, rc, skip, mark, fast)


def tile_records(reads, k, span, rc, skip=None, mark=False, fast=False):
    L = np.asarray(reads).shape[1]
    return _fixed(reads, 0, span, (L - k + 1) // span, k + span - 1, rc, skip, mark, fast)


def remainder_records(reads, k, span, rc, skip=None, mark=False, fast=False):
    L = np.asarray(reads).shape[1]
    W = L - k + 1
    return _fixed(reads, (W // span) * span, 1, W % span, k, rc, skip, mark, fast)


# ---- reads of varying length: `seqs` is a list of strings, none shorter than k --------------------------------------------------------
def _prefix(counts):
    return np.concatenate(([0], np.cumsum(np.asarray(counts, dtype=np.int64)))).astype(np.int64)


def window_prefix(seqs, k):
    return _prefix([len(s) - k + 1 for s in seqs])


def _var(seqs, starts_of, length, rc, mark):
    values, marked, counts = [], [], []
    for s in seqs:
        starts = starts_of(len(s))
        counts.append(len(starts))
        for w in starts:
            v, m = window_record(s, w, length, rc, mark)
            values.append(v)
            marked.append(m)
    return format_words(values, marked, words_for(length)), _prefix(counts)


def var_records(seqs, k, rc, mark=False):
    return _var(seqs, lambda n: range(n - k + 1), k, rc, mark)[0]


def var_tile_records(seqs, k, span, rc, mark=False):
    """-> (records, tiles before each read [n + 1], windows before each read [n + 1])"""
    rec, pref = _var(seqs, lambda n: range(0, ((n - k + 1) // span) * span, span), k + span - 1, rc, mark)
    return rec, pref, window_prefix(seqs, k)


def var_remainder_records(seqs, k, span, rc, mark=False):
    """-> (records, left-over windows before each read [n + 1], windows before each read [n + 1])"""
    rec, pref = _var(seqs, lambda n: range(((n - k + 1) // span) * span, n - k + 1), k, rc, mark)
    return rec, pref, window_prefix(seqs, k)


# ---- the tile shapes both test files walk -----------------------------------------------------------------------------------------
# (k, span, tiles per read at a read of at most 256 bases, tiles per read at a longer one): 31, 32, 63, 64, 64 and 95 bases a tile
TILE_SPANS = [(16, 16, 8, 17), (31, 2, 60, 120), (31, 33, 3, 7), (32, 33, 3, 7), (63, 2, 44, 100), (63, 33, 2, 6)]


def tile_cases(long_reads):
    """(k, span, L): for every span above, windows per read that leave 0, 1 and span - 1 over, and L = k + span - 2 (no whole tile)"""
    out = []
    for k, span, few, many in TILE_SPANS:
        for rest in sorted({0, 1, span - 1}):
            out.append((k, span, k - 1 + span * (many if long_reads else few) + rest))
        if not long_reads:
            out.append((k, span, k + span - 2))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def random_reads(rng, n, L):
    """[n, L] ASCII"""
    return _ASCII[rng.integers(0, 4, size=(n, L), dtype=np.uint8)]


def random_seq(rng, length):
    return bytes(_ASCII[rng.integers(0, 4, size=length, dtype=np.uint8)]).decode()


def _noisy_pad(packed_rows, L, rng):
    """the bits of a read's last byte that hold no base: random instead of zero (nothing may depend on them)"""
    pad_bits = 2 * ((-L) % 4)
    if pad_bits:
        packed_rows[:, -1] |= rng.integers(0, 1 << pad_bits, size=packed_rows.shape[0], dtype=np.uint8)
    return packed_rows


def pack_fixed(reads, rng, skip=None):
    """[n, L] ASCII -> [n * ceil(L/4)] uint8, pad bits random; the rows of skipped reads are random bytes"""
    reads = np.asarray(reads, dtype=np.uint8)
    p = _noisy_pad(np.ascontiguousarray(pack_reads_ascii(reads)), reads.shape[1], rng)
    if skip is not None:
        sk = np.asarray(skip, dtype=bool)
        p[sk] = rng.integers(0, 256, size=(int(sk.sum()), p.shape[1]), dtype=np.uint8)
    return p.reshape(-1)


def pack_var(seqs, rng=None):
    """-> (packed uint8, byte_off int64 [n + 1], lens int32 [n]): every read starts on a byte, the buffer ends with the last read's
    last byte; rng: random pad bits"""
    parts, off = [], [0]
    for s in seqs:
        row = pack_reads_ascii(np.frombuffer(s.encode(), np.uint8)[None, :]).copy()
        if rng is not None:
            row = _noisy_pad(row, len(s), rng)
        parts.append(row.reshape(-1))
        off.append(off[-1] + row.size)
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return packed, np.asarray(off, np.int64), np.asarray([len(s) for s in seqs], np.int32)
