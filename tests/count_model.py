"""What a level counted by sorting must give (records_to_edges_sorted, katome_dev_count_records), as a dictionary: plain Python
integers, keys as numbers of 2k bits (the first base in the highest bits, as helpers.kmer_to_int), no numpy near a weight.

Where the rules come from -- none of them from lds_count.hip:
  * both strands, the doubled self-complementary k-mer and the threshold: the reference's build and Clean::remove_weak_edges, as the
    oracle restates them; tests/test_count_model_host.py holds this model against oracle.build_ascii on literal reads.
  * sums wrap in 32 bits: the oracle never gets near 2^32, so this one rule is taken from the sentence at table.hip:8 ("Weights are
    u32 and wrap like EdgeWeight") and pinned on three literal sums in the same test file.  The doubling of a self-complementary
    k-mer is a sum like any other and wraps the same way; the threshold looks at the weight an edge ends up with.
"""
from helpers import int_to_words

M32 = (1 << 32) - 1
# one byte's four bases in reverse order
_REV4 = bytes(((b & 3) << 6) | (((b >> 2) & 3) << 4) | (((b >> 4) & 3) << 2) | (b >> 6) for b in range(256))


def revcomp(key, k):
    """the reverse complement of a k-mer given as a number of 2k bits"""
    nb = (2 * k + 7) // 8
    flipped = (key ^ ((1 << (2 * k)) - 1)).to_bytes(nb, "little")          # complemented; read big-endian below: the bytes reversed
    return int.from_bytes(flipped.translate(_REV4), "big") >> (8 * nb - 2 * k)


def canonical(key, k):
    """one orientation per k-mer for the records of a both-strand count (which one does not matter to count())"""
    return min(key, revcomp(key, k))


def sums(records, weights=None):
    """{key: sum of its records' weights mod 2^32}; weights None: every record counts once"""
    out = {}
    if weights is None:
        for key in records:
            out[key] = (out.get(key, 0) + 1) & M32
    else:
        assert len(weights) == len(records)
        for key, w in zip(records, weights):
            w = int(w)
            assert 0 <= w <= M32
            out[key] = (out.get(key, 0) + w) & M32
    return out


def count(records, weights, k, rc, min_weight):
    """-> the sorted list of (key, weight) edges.  rc: the records hold one orientation of a k-mer only (ValueError otherwise: the
    count's contract, and two records of one k-mer in both orientations would leave it twice)"""
    total = sums([int(x) for x in records], weights)
    out = []
    for key, w in total.items():
        if not rc:
            edges = ((key, w),)
        else:
            other = revcomp(key, k)
            if other == key:
                edges = ((key, (2 * w) & M32),)
            elif other in total:
                raise ValueError("both orientations of one k-mer among the records")
            else:
                edges = ((key, w), (other, w))
        out.extend(e for e in edges if e[1] >= min_weight)
    return sorted(out)


def n_distinct(records):
    return len(set(int(x) for x in records))


def owners(keys, k, n_parts):
    """owner of every key (one word) by the hash of its core, the middle k - 2 bases: the library's own host function"""
    from katome_amd import device as kd
    return [kd.key_owner(int_to_words(int(key), 1), n_parts, core=(2, k - 2)) for key in keys]
