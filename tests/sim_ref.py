"""pfq_tree_similarity restated in numpy over an oracle tree (include/pfq.h "genome similarity"): the shared set bits of every
pair of listed leaf filters, each filter's set bits, and the doubles derived from them; and the line SIMILARITY.tsv holds for a
pair.  Nothing here knows how the library computes any of it."""
import math

import numpy as np

HEADER = "#genome_a\tgenome_b\tbits_a\tbits_b\tshared_bits\tkmers_a\tkmers_b\tshared_kmers\tjaccard\tcontainment_a\tcontainment_b\tani"
INT_KEYS = ("shared_bits", "bits_a", "bits_b")
FLOAT_KEYS = ("kmers_a", "kmers_b", "shared_kmers", "jaccard")


def leaf_rows(ot):
    """The filter words of the tree's leaves, in leaf order: uint64 [n_leaves, n_words]."""
    return np.stack([ot.bits[ot.filter_of[v]] for v in ot.leaves_dfs()]) if ot.root >= 0 else np.zeros((0, ot.n_words), np.uint64)


def popcount(words):
    """Set bits per row of a uint64 array [.., n_words]."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).sum(axis=-1, dtype=np.uint64)


def below(words, nbits):
    """The rows with every bit index >= nbits cleared (Lsb0 words)."""
    out = np.array(words, dtype=np.uint64, copy=True)
    if nbits % 64:
        out[..., -1] &= np.uint64((1 << (nbits % 64)) - 1)
    return out


def shared_bits(ra, rb, chunk_words=2048):
    """popcount(ra[i] & rb[j]) for all i, j as a product of 0/1 matrices, a stretch of words at a time: a stretch's sums stay
    below 2^24, so float32 holds them exactly."""
    total = np.zeros((len(ra), len(rb)), dtype=np.int64)
    if len(ra) and len(rb):
        for w in range(0, ra.shape[1], chunk_words):
            a = np.unpackbits(np.ascontiguousarray(ra[:, w:w + chunk_words]).view(np.uint8), axis=1).astype(np.float32)
            b = np.unpackbits(np.ascontiguousarray(rb[:, w:w + chunk_words]).view(np.uint8), axis=1).astype(np.float32)
            total += np.rint(a @ b.T).astype(np.int64)
    assert total.max(initial=0) < 2 ** 32
    return total.astype(np.uint32)


def kmers(x, m, h):
    """n(x): the distinct items behind x set bits of a filter of m bits and h hashes; a full filter is not estimable: 0.0."""
    return 0.0 if x >= m else -(m / h) * math.log1p(-x / m)


def derive(shared, bits_a, bits_b, m, h):
    """The doubles of pfq_similarity from its integers."""
    n_a, n_b = len(bits_a), len(bits_b)
    out = {"kmers_a": np.array([kmers(int(x), m, h) for x in bits_a], dtype=np.float64),
           "kmers_b": np.array([kmers(int(x), m, h) for x in bits_b], dtype=np.float64),
           "shared_kmers": np.zeros((n_a, n_b)), "jaccard": np.zeros((n_a, n_b))}
    for i in range(n_a):
        for j in range(n_b):
            a, b = int(bits_a[i]), int(bits_b[j])
            u = a + b - int(shared[i, j])
            if a >= m or b >= m or u >= m:
                continue
            nu = kmers(u, m, h)
            sh = max(0.0, out["kmers_a"][i] + out["kmers_b"][j] - nu)
            out["shared_kmers"][i, j] = sh
            out["jaccard"][i, j] = sh / nu if nu > 0.0 else 0.0
    return out


def similarity_rows(rows_a, rows_b, m, h):
    """What pfq_tree_similarity returns for filter rows rows_a [n_a, n_words] and rows_b [n_b, n_words] of m bits, h hashes."""
    ra, rb = below(rows_a, m), below(rows_b, m)
    shared = shared_bits(ra, rb)
    out = {"shared_bits": shared, "bits_a": popcount(ra) if len(ra) else np.zeros(0, np.uint64),
           "bits_b": popcount(rb) if len(rb) else np.zeros(0, np.uint64)}
    out.update(derive(shared, out["bits_a"], out["bits_b"], m, h))
    return out


def similarity(ot_a, ot_b=None, leaves_a=None, leaves_b=None):
    """tree.similarity(other, leaves_a, leaves_b) over oracle trees (ot_b None: ot_a; a list None: all leaves)."""
    ot_b = ot_a if ot_b is None else ot_b
    assert (ot_a.kmer_size, ot_a.nbits, ot_a.num_hashes, ot_a.seed1, ot_a.seed2) == (ot_b.kmer_size, ot_b.nbits, ot_b.num_hashes, ot_b.seed1, ot_b.seed2)
    ra, rb = leaf_rows(ot_a), leaf_rows(ot_b)
    if leaves_a is not None:
        ra = ra[np.asarray(leaves_a, dtype=np.int64)]
    if leaves_b is not None:
        rb = rb[np.asarray(leaves_b, dtype=np.int64)]
    return similarity_rows(ra, rb, ot_a.nbits, ot_a.num_hashes)


def sub(ref, ia, ib):
    """The part of an all x all result that the lists ia, ib ask for."""
    ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    out = {k: ref[k][np.ix_(ia, ib)] for k in ("shared_bits", "shared_kmers", "jaccard")}
    out.update({"bits_a": ref["bits_a"][ia], "kmers_a": ref["kmers_a"][ia], "bits_b": ref["bits_b"][ib], "kmers_b": ref["kmers_b"][ib]})
    return out


def same(got, want, tag=None):
    """A similarity() dict of the library against one of this module: integers exactly; the doubles — one formula applied to
    identical integers on both sides, so only libm's rounding differs — at relative 1e-9."""
    for k in INT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (tag, k)
    for k in FLOAT_KEYS:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (tag, k)
        assert np.allclose(got[k], want[k], rtol=1e-9, atol=0.0), (tag, k)


def pair_values(ref, i, j, k):
    """The twelve columns of SIMILARITY.tsv for pair (i, j) of `ref`, names left out: three ints and seven doubles."""
    ka, kb, sh, jac = (float(ref["kmers_a"][i]), float(ref["kmers_b"][j]), float(ref["shared_kmers"][i, j]), float(ref["jaccard"][i, j]))
    ca, cb = (sh / ka if ka > 0.0 else 0.0), (sh / kb if kb > 0.0 else 0.0)
    ani = 1.0 + math.log(2.0 * jac / (1.0 + jac)) / k if jac > 0.0 else 0.0
    return (int(ref["bits_a"][i]), int(ref["bits_b"][j]), int(ref["shared_bits"][i, j])), (ka, kb, sh, jac, ca, cb, ani)


def tsv_line(name_a, name_b, ref, i, j, k):
    """k-mer counts as %.1f, ratios as %.6f."""
    ints, (ka, kb, sh, jac, ca, cb, ani) = pair_values(ref, i, j, k)
    return "\t".join([name_a, name_b] + [str(x) for x in ints] + [f"{x:.1f}" for x in (ka, kb, sh)] + [f"{x:.6f}" for x in (jac, ca, cb, ani)])


def max_containment(ref, i, j, k):
    v = pair_values(ref, i, j, k)[1]
    return max(v[4], v[5])
