"""The texts tests/test_format_cpu.py and tests/test_gpu_format.py format: every shape of header, line end, sequence and quality
the rules of pfq.h "text output" distinguish.  Built once, from fixed seeds; nothing changes them."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
BLOCKS = (1, 2, 7, 64, 100, 8192)


def first_indices(block):
    return sorted({0, 3, block - 1, (1 << 40) + 5})


def dna(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].tobytes()


def header_of(i):
    """Record i's header without its marker: ids that repeat inside a block of 7 or more (empty, "a"), ids that differ only
    behind byte 8 or in their last byte, a tab that ends a FASTA id and not a FASTQ one."""
    special = {3: b"", 5: b"   ", 8: b"a x", 9: b"a y", 12: b"abcdefgh1", 13: b"abcdefgh2", 14: b"one_long_prefix_one_long_prefix_A",
               15: b"one_long_prefix_one_long_prefix_B tail", 17: b"t\tb x", 18: b"t\tc", 20: b"trailing blanks \t "}
    return special.get(i, b"r%d some words /1" % i if i % 3 else b"r%d" % i)


def odd_reads(rng):
    """Sequence lengths 0 .. 40 (every alignment of source and destination), 5000 bases, lower case, bytes of 0x80 and above."""
    out = [dna(rng, n) for n in range(41)] + [dna(rng, 5000)]
    out += [dna(rng, 33).lower(), b"acgtNnXx@`{[\x7f\x80\xe1\xfa\xffzZaA" + dna(rng, 9), bytes(range(0x61, 0x7b)) + bytes(range(0xe1, 0xfb)) + b"`{"]
    return out


def fastq(reads, eol=b"\n", final_newline=True):
    out = []
    for i, r in enumerate(reads):
        qual = (b"@" if i % 4 == 1 else b"I") + bytes(33 + (j * 7 + i) % 60 for j in range(max(len(r), 1) - 1))  # (some begin with '@')
        out.append(eol.join([b"@" + header_of(i), r, b"+" if i % 2 else b"+" + header_of(i), qual + (b"  " if i % 5 == 2 else b"")]) + eol)
    data = b"".join(out)
    return data if final_newline else data[:-len(eol)]


def fasta(reads, eol=b"\n", final_newline=True, width=60):
    out = []
    for i, r in enumerate(reads):
        lines = [r[j:j + width] for j in range(0, len(r), width)]  # (multi-line records; an empty sequence has no line)
        out.append(eol.join([b">" + header_of(i)] + lines) + eol)
    data = b"".join(out)
    return data if final_newline else data[:-len(eol)]


def texts(reads):
    """{name: (data, is_fastq)}: `reads` in every dress."""
    return {"fastq": (fastq(reads), True), "fastq_crlf": (fastq(reads, b"\r\n"), True), "fastq_unterminated": (fastq(reads, final_newline=False), True),
            "fasta": (fasta(reads), False), "fasta_crlf": (fasta(reads, b"\r\n"), False), "fasta_unterminated": (fasta(reads, final_newline=False), False)}


SMALL = {"empty": (b"", True), "empty_fasta": (b"", False), "one": (b"@q w\nACGTacgt\n+\n!!!!!!!!\n", True), "one_fasta": (b">q\tw\nACGTacgt\nGG\n", False),
         "empty_id_twice": (b"@\nAC\n+\n!!\n@ x\nGG\n+\n##\n@z\nTT\n+\n$$\n", True),
         "same_id": (b"@a x\nAC\n+\n!!\n@a y\nGG\n+\n##\n@b\nTT\n+\n$$\n@c\n\n+\n%\n", True)}
