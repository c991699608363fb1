"""The rules of pfq_text_parse (include/pfq.h "text") in plain Python: what the device parser must return for a piece of plain
FASTA / FASTQ text whose first byte is claimed to begin a record.  tests/test_text_cpu.py holds these rules against the
sequential readers of tests/test_ingest.py; tests/test_gpu_text.py holds the device against these rules."""

BLANK = b" \t\n\v\f\r"
END, LIMIT, MORE, SLOW = "end", "limit", "more", "slow"


def considered_lines(data: bytes, final: bool):
    """[(begin, line without its newline)] of the lines the parser may look at: every run ended by a newline, and an
    unterminated last run only if the text ends where the file ends."""
    lines, pos = [], 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        if nl < 0:
            if final:
                lines.append((pos, data[pos:]))
            break
        lines.append((pos, data[pos:nl]))
        pos = nl + 1
    return lines


def scan(data: bytes, fastq: bool, limit=None, final: bool = True):
    """-> (sequences, rec_begin, consumed, stop): the records taken, rec_begin = the byte offset of each one's header line and
    then consumed (len(sequences) + 1 entries)."""
    if limit is None:
        limit = 1 << 64
    lines = considered_lines(data, final)
    n = len(lines)
    seqs, begins = [], []

    def begin_of(i):  # where line i begins; behind the considered lines: where they end
        if i < n:
            return lines[i][0]
        return min(lines[-1][0] + len(lines[-1][1]) + 1, len(data)) if n else 0

    if fastq:
        r = 0
        while True:
            b = begin_of(4 * r)
            if b == len(data):
                stop = END
            elif 4 * r == n:
                stop = MORE
            elif b >= limit:
                stop = LIMIT
            elif n - 4 * r < 4:
                stop = SLOW if final else MORE
            else:
                l0, l1, l2, l3 = (lines[4 * r + j][1] for j in range(4))
                plain = l0[:1] == b"@" and l1[:1] != b"+" and l2[:1] == b"+" and l3.rstrip(BLANK) != b""
                if plain:
                    seqs.append(l1.rstrip(BLANK))
                    begins.append(b)
                    r += 1
                    continue
                stop = SLOW
            return seqs, begins + [b], b, stop
    if not data:
        return [], [0], 0, END
    if data[:1] != b">":
        return [], [0], 0, SLOW
    headers = [i for i in range(n) if lines[i][1][:1] == b">"]
    if not headers:                      # the header line itself is not complete yet
        return [], [0], 0, (LIMIT if limit == 0 else MORE)
    for j, h in enumerate(headers):
        b = lines[h][0]
        last = j + 1 == len(headers)
        if b >= limit:
            return seqs, begins + [b], b, LIMIT
        if last and not final:
            return seqs, begins + [b], b, MORE
        nxt = n if last else headers[j + 1]
        seqs.append(b"".join(lines[i][1].rstrip(BLANK) for i in range(h + 1, nxt)))
        begins.append(b)
    return seqs, begins + [len(data)], len(data), END
