"""The rules the device parser implements (tests/text_ref.py) against the sequential readers restated in tests/test_ingest.py.
CPU only.  For every input: the records the rules take are a prefix of the sequential reader's, and the sequential reader
started at `consumed` yields the rest and the same error — so a caller that hands the rest to the sequential reader gets
exactly what the sequential reader alone would have given, malformed input included."""
import pytest

import test_ingest as ing
import text_ref

ADVERSARIAL = b"".join(b"@r%d\n@AAA%d\nCCCC\nGGGG\n+\n@III%d\nIIII\n+III\n" % (i, i % 10, i % 10) for i in range(300))
MALFORMED_TAILS = [b"@x\nACGT\n", b"@x\nACGT\n+\n", b"@x\n\n+\n\n@y\nAC\n+\n!!\n", b"ACGT\n", b"\n",
                   b"@x\nAC\nGT\n+\n!!!!\n@y\nAC\n+\n!!\n"]


def sequential(data: bytes, fastq: bool):
    """(sequences, error or None) of the sequential reader."""
    if fastq:
        recs, bad = ing.parse_fastq(data, partial=True)
        return [r[2] for r in recs], bad
    lines, i, seqs = ing._lines(data), 0, []
    while i < len(lines):           # parse_fasta, delivering what came before a malformed record
        if lines[i][:1] != b">":
            return seqs, "Expected >"
        i += 1
        seq = b""
        while i < len(lines) and lines[i][:1] != b">":
            seq += lines[i].rstrip()
            i += 1
        seqs.append(seq)
    return seqs, None


def check_whole(data: bytes, fastq: bool):
    want, why = sequential(data, fastq)
    seqs, begins, consumed, stop = text_ref.scan(data, fastq)
    assert seqs == want[:len(seqs)]
    assert len(begins) == len(seqs) + 1 and begins[-1] == consumed and begins == sorted(begins)
    assert stop in (text_ref.END, text_ref.SLOW)      # no limit, the whole file: nothing is ever "more" or "limit"
    assert (stop == text_ref.END) == (consumed == len(data))
    rest, why_rest = sequential(data[consumed:], fastq)
    assert seqs + rest == want and why_rest == why
    return len(seqs), len(want)


def chained(data: bytes, fastq: bool, limit: int):
    """Pieces as the CLI cuts them: a window of `limit` bytes and some slack from the proven position, final only when it reaches
    the end of the file; "more" widens the slack, "slow" hands the rest to the sequential reader."""
    out, pos, slack = [], 0, 16
    while True:
        window = data[pos:pos + limit + slack]
        final = pos + len(window) == len(data)
        seqs, begins, consumed, stop = text_ref.scan(window, fastq, limit, final)
        for b, s in zip(begins, seqs):
            assert b < limit
        out += seqs
        pos += consumed
        if stop == text_ref.END:                      # the window is used up: the file's end, or just a window that ends at a record's end
            assert consumed == len(window)
            if final:
                return out, None
            continue
        if stop == text_ref.SLOW:
            rest, why = sequential(data[pos:], fastq)
            return out + rest, why
        if stop == text_ref.MORE:
            assert not final
            slack *= 2
        else:
            assert consumed >= limit
            slack = 16


@pytest.mark.parametrize("multiline,crlf,final_newline", [(False, False, True), (False, True, True), (False, False, False),
                                                          (True, False, True), (True, True, True), (True, False, False)])
def test_fastq_generators(multiline, crlf, final_newline):
    data = ing.tricky_fastq(200, multiline=multiline, crlf=crlf, final_newline=final_newline)
    taken, total = check_whole(data, True)
    if not multiline:
        assert taken == total == 200                 # single-line files are taken whole
    else:
        assert taken < total                         # ... multi-line files stop at the first multi-line record
    for limit in (1, 17, 200, 4096):
        assert chained(data, True, limit) == sequential(data, True)


@pytest.mark.parametrize("crlf", [False, True])
def test_fasta_generators(crlf):
    data = ing.tricky_fasta(80, crlf=crlf)
    assert check_whole(data, False) == (80, 80)
    for limit in (1, 17, 200, 4096):
        assert chained(data, False, limit) == sequential(data, False)


def test_adversarial_three_line_file():
    taken, total = check_whole(ADVERSARIAL, True)
    assert (taken, total) == (0, 300)
    for start in (ADVERSARIAL.index(b"@III1"), ADVERSARIAL.index(b"@AAA2")):   # false record starts a guess may land on
        check_whole(ADVERSARIAL[start:], True)
    for limit in (17, 4096):
        assert chained(ADVERSARIAL, True, limit) == sequential(ADVERSARIAL, True)


@pytest.mark.parametrize("tail", MALFORMED_TAILS)
def test_malformed_tails(tail):
    good = ing.tricky_fastq(50, multiline=False)
    data = good + tail
    want, why = sequential(data, True)
    assert why is not None
    taken, total = check_whole(data, True)
    assert taken >= 50
    for limit in (1, 17, 200, 4096):
        assert chained(data, True, limit) == (want, why)
    check_whole(tail, True)


def test_malformed_fasta():
    for data in (b"ACGT\n>a\nAC\n", b"\n>a\nAC\n", b" >a\nAC\n"):
        assert text_ref.scan(data, False) == ([], [0], 0, text_ref.SLOW)
        check_whole(data, False)


def test_unequal_lengths_and_empty_sequence():
    data = b"@a 1\nACGTACGT\n+\n!!!\n@b\nAC\n+\nIIIIIIII\n@c\n\n+\n!\n@d\nAC  \r\n+\r\n \t\r\n"
    seqs, begins, consumed, stop = text_ref.scan(data, True)
    assert seqs == [b"ACGTACGT", b"AC", b""] and stop == text_ref.SLOW and consumed == data.index(b"@d")
    check_whole(data, True)


def test_stops():
    fq = b"@a\nAC\n+\n!!\n@b\nGT\n+\n##\n"
    assert text_ref.scan(b"", True) == ([], [0], 0, text_ref.END)
    assert text_ref.scan(b"", False, 0) == ([], [0], 0, text_ref.END)
    assert text_ref.scan(fq, True, 0) == ([], [0], 0, text_ref.LIMIT)
    assert text_ref.scan(fq, True, 1) == ([b"AC"], [0, 11], 11, text_ref.LIMIT)
    assert text_ref.scan(fq, True, 12) == ([b"AC", b"GT"], [0, 11, 22], 22, text_ref.END)
    assert text_ref.scan(fq[:-1], True, None, False) == ([b"AC"], [0, 11], 11, text_ref.MORE)
    assert text_ref.scan(fq[:-1], True, None, True) == ([b"AC", b"GT"], [0, 11, 21], 21, text_ref.END)
    assert text_ref.scan(fq[:14], True, None, True) == ([b"AC"], [0, 11], 11, text_ref.SLOW)
    assert text_ref.scan(b"@a", True, None, False) == ([], [0], 0, text_ref.MORE)
    fa = b">a\nAC\nGT\n>b\n\nT \n"
    assert text_ref.scan(fa, False) == ([b"ACGT", b"T"], [0, 9, 16], 16, text_ref.END)
    assert text_ref.scan(fa, False, None, False) == ([b"ACGT"], [0, 9], 9, text_ref.MORE)
    assert text_ref.scan(fa, False, 9) == ([b"ACGT"], [0, 9], 9, text_ref.LIMIT)
    assert text_ref.scan(fa, False, 0) == ([], [0], 0, text_ref.LIMIT)
    assert text_ref.scan(b">", False, None, False) == ([], [0], 0, text_ref.MORE)
    assert text_ref.scan(b">", False) == ([b""], [0, 1], 1, text_ref.END)
