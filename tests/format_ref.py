"""The rules of pfq_text_format (include/pfq.h "text output") in plain Python, on top of text_ref.scan: what the device formatter
must return for a piece of plain FASTA / FASTQ text, the hit rows of its records and the leaves' names — the two streams and
the runs of records it leaves to the caller.  Beside it, the reference's own decision (result_map.rs:20-45): a map id -> genomes
per block of records.  tests/test_format_cpu.py holds the first against the second; tests/test_gpu_format.py holds the device
against the first."""
import text_ref

BLANK = text_ref.BLANK
HEAD, TAIL, REPEATED_ID = "head", "tail", "repeated_id"
BLOCK_MAX = 8192
_UPPER = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))


def records(data: bytes, fastq: bool, limit=None, final: bool = True):
    """[(id, sequence, quality or None)] of the records the parser takes from data."""
    seqs, begins, _, _ = text_ref.scan(data, fastq, limit, final)
    out = []
    for r, seq in enumerate(seqs):
        lines = data[begins[r]:begins[r + 1]].split(b"\n")
        header = lines[0].rstrip(BLANK)
        seps = b" " if fastq else BLANK
        i = 1
        while i < len(header) and header[i] not in seps:
            i += 1
        out.append((header[1:i], seq, lines[3].rstrip(BLANK) if fastq else None))
    return out


def put_record(rec, leaves, names) -> bytes:
    """One record as the CLI's put_record writes it; leaves: the genomes printed behind the id (none: the record is unmapped)."""
    rid, seq, qual = rec
    out = (b">" if qual is None else b"@") + rid
    if len(leaves):
        out += b" |" + b",".join(names[int(l)] for l in leaves)
    out += b"\n" + seq.translate(_UPPER) + b"\n"
    if qual is not None:
        out += b"+\n" + qual + b"\n"
    return out


def dict_block(recs, rows, names, pos=True, neg=True):
    """One result block the reference's way: id -> the set of its records' genomes (printed in leaf order); a record is mapped
    when its id is in the map.  -> (pos bytes, neg bytes)."""
    genomes = {}
    for (rid, _, _), row in zip(recs, rows):
        if len(row):
            genomes.setdefault(rid, set()).update(int(l) for l in row)
    p, n = [], []
    for rec in recs:
        if rec[0] in genomes:
            if pos:
                p.append(put_record(rec, sorted(genomes[rec[0]]), names))
        elif neg:
            n.append(put_record(rec, (), names))
    return b"".join(p), b"".join(n)


def dict_all(recs, rows, names, first_index, block, pos=True, neg=True):
    """The whole input block by block, record r lying in block (first_index + r) // block."""
    p, n, r = [], [], 0
    while r < len(recs):
        e = min(len(recs), r + block - (first_index + r) % block)
        a, b = dict_block(recs[r:e], rows[r:e], names, pos, neg)
        p.append(a)
        n.append(b)
        r = e
    return b"".join(p), b"".join(n)


def format_ref(recs, rows, names, first_index=0, block=100, pos=True, neg=True):
    """-> {"pos", "neg", "pos_records", "neg_records", "left": [(first, count, pos_at, neg_at, why)]} by the rules of pfq.h."""
    assert 1 <= block <= BLOCK_MAX and (pos or neg)
    n = len(recs)
    head = (block - first_index % block) % block
    n_whole = (n - head) // block if head < n else 0
    if not n_whole:
        head = n
    p, q, left, n_pos, n_neg = bytearray(), bytearray(), [], 0, 0
    if head:
        left.append((0, head, 0, 0, HEAD))
    for b in range(n_whole):
        r0 = head + b * block
        if len({recs[r][0] for r in range(r0, r0 + block)}) < block:
            left.append((r0, block, len(p), len(q), REPEATED_ID))
            continue
        for r in range(r0, r0 + block):
            if len(rows[r]):
                if pos:
                    p += put_record(recs[r], rows[r], names)
                    n_pos += 1
            elif neg:
                q += put_record(recs[r], (), names)
                n_neg += 1
    tail = head + n_whole * block
    if tail < n:
        left.append((tail, n - tail, len(p), len(q), TAIL))
    return {"n_records": n, "pos": bytes(p), "neg": bytes(q), "pos_records": n_pos, "neg_records": n_neg, "left": left}


def splice(res, recs, rows, names, first_index, block, pos=True, neg=True):
    """The streams of a format result with the left runs formatted by dict_block, block by block, and spliced in at pos_at /
    neg_at: the whole input's output in record order."""
    p, q, pc, qc = [], [], 0, 0
    for first, count, pos_at, neg_at, _ in res["left"]:
        a, b = dict_all(recs[first:first + count], rows[first:first + count], names, first_index + first, block, pos, neg)
        p += [res["pos"][pc:pos_at], a]
        q += [res["neg"][qc:neg_at], b]
        pc, qc = pos_at, neg_at
    return b"".join(p) + res["pos"][pc:], b"".join(q) + res["neg"][qc:]
