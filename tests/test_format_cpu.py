"""tests/format_ref.py against the reference's own decision: the streams format_ref gives for the whole plain blocks, with the
runs it leaves formatted through a per-block map id -> genomes and spliced in at pos_at / neg_at, must be byte for byte what
that map gives for the whole input.  CPU only."""
import numpy as np
import pytest

import format_cases as fc
import format_ref as fr

NAMES = [b"g%d" % i + b"n" * ((i * 7) % 40) for i in range(130)]


def random_rows(rng, n, n_leaves):
    """Hit rows as a query call gives them: ascending, no duplicates; empty, single, a few, more than 64, every leaf."""
    rows = []
    for _ in range(n):
        kind = int(rng.integers(0, 10))
        size = (0, 0, 0, 0, 1, 1, 2, 5, 70, n_leaves)[kind]
        rows.append(np.sort(rng.choice(n_leaves, min(size, n_leaves), replace=False)).astype(np.uint32))
    return rows


def cases():
    rng = np.random.default_rng(20261019)
    reads = fc.odd_reads(rng) + [fc.dna(rng, int(n)) for n in rng.integers(30, 300, 260)]
    out = dict(fc.texts(reads))
    out.update(fc.SMALL)
    return out


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_spliced_streams_equal_the_block_map(name):
    data, fastq = CASES[name]
    recs = fr.records(data, fastq)
    rng = np.random.default_rng(len(data))
    for n_leaves in (12, 130):
        rows = random_rows(rng, len(recs), n_leaves)
        for block in fc.BLOCKS:
            for first in fc.first_indices(block):
                for pos, neg in ((True, True), (True, False), (False, True)):
                    res = fr.format_ref(recs, rows, NAMES, first, block, pos, neg)
                    want = fr.dict_all(recs, rows, NAMES, first, block, pos, neg)
                    assert fr.splice(res, recs, rows, NAMES, first, block, pos, neg) == want, (name, n_leaves, block, first, pos, neg)
                    if block == 1:
                        assert res["left"] == []                      # a block of one record is always whole and plain
                        assert (res["pos"], res["neg"]) == want


def test_the_cases_hold_what_they_claim():
    recs = fr.records(*CASES["fastq"])
    ids = [r[0] for r in recs]
    assert ids[3] == ids[5] == b"" and ids[8] == ids[9] == b"a" and ids[12] != ids[13] and ids[12][:8] == ids[13][:8]
    assert ids[14][:-1] == ids[15][:-1] and ids[14] != ids[15] and (ids[17], ids[18]) == (b"t\tb", b"t\tc") and ids[20] == b"trailing"
    assert sorted({len(r[1]) for r in recs[:41]}) == list(range(41)) and len(recs[41][1]) == 5000
    assert any(r[2][:1] == b"@" for r in recs) and all(r[2] and r[2] == r[2].rstrip() for r in recs)
    fa = fr.records(*CASES["fasta"])
    assert [r[1] for r in fa] == [r[1] for r in recs] and (fa[17][0], fa[18][0]) == (b"t", b"t") and all(r[2] is None for r in fa)
    for name in ("fastq_crlf", "fastq_unterminated", "fasta_crlf", "fasta_unterminated"):
        assert fr.records(*CASES[name]) == (recs if CASES[name][1] else fa), name
    assert fr.put_record((b"i", b"az`{AZ\x80\xe1\xff", b"q"), [1, 0], [b"x", b"y"]) == b"@i |y,x\nAZ`{AZ\x80\xe1\xff\n+\nq\n"
    assert fr.put_record((b"", b"", None), [], []) == b">\n\n"


@pytest.mark.parametrize("block", fc.BLOCKS)
def test_head_and_tail_accounting(block):
    recs = fr.records(*CASES["fastq"])
    n = len(recs)
    rows = [np.zeros(0, dtype=np.uint32)] * n
    for first in fc.first_indices(block):
        left = fr.format_ref(recs, rows, NAMES, first, block)["left"]
        edge = [x for x in left if x[4] != fr.REPEATED_ID]
        head = (block - first % block) % block
        if head >= n or (n - head) // block == 0:
            assert left == [(0, n, 0, 0, fr.HEAD)]
            continue
        n_whole = (n - head) // block
        want = ([(0, head, fr.HEAD)] if head else []) + ([(head + n_whole * block, n - head - n_whole * block, fr.TAIL)] if (n - head) % block else [])
        assert [(x[0], x[1], x[4]) for x in edge] == want
        for first_r, count, _, _, why in left:                         # whole blocks begin on a boundary of the global index
            if why != fr.HEAD:
                assert (first + first_r) % block == 0
            if why == fr.REPEATED_ID:
                assert count == block and len({recs[r][0] for r in range(first_r, first_r + count)}) < block
        covered = sum(x[1] for x in left)
        assert covered == sum(x[1] for x in edge) + block * sum(x[4] == fr.REPEATED_ID for x in left)
