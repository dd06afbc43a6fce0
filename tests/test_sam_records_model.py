"""A plain model of gdx_sam_records_many (include/gdx_experimental.h "SAM records"): one SAM record per read, written from the
definition, pinned on the header's worked examples and on hand-written cases, and checked independently on random alignments of
align_model: text[begin:end] is rebuilt from SEQ, CIGAR and MD alone.  tests/test_gpu_sam_records.py holds the device against it."""
import os
import re

import numpy as np

from genedex_amd import alphabet as alph
from test_align_model import align_model
from test_edit_distance_model import NO_END
from test_mate_rescue_model import random_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = alph.ascii_dna_with_n()
NONE = 0xFFFFFFFF
SINGLE, PAIRED = 0, 1
BAD_RECORD = 1
MAX_RUN_SUM = 1 << 24
OPS = "MIDNSHP=X"
INS, DEL, EQ, DIFF = 1, 2, 7, 8


def default_table(alphabet):
    """dense_to_io of a call that passes NULL: entry c >= 1 the smallest byte of dense code c, entry 0 (a text symbol outside
    1..4) the smallest byte of the alphabet's one dense code above 4, '?' where there is none or several"""
    dense = np.asarray(alphabet.io_to_dense_table, dtype=np.int64)
    tab = bytearray(b"?" * 16)
    for c in range(1, 16):
        where = np.flatnonzero(dense == c)
        if where.size:
            tab[c] = int(where[0])
    others = sorted(set(int(d) for d in dense if d > 4))
    if len(others) == 1:
        tab[0] = int(np.flatnonzero(dense == others[0])[0])
    return bytes(tab)


def words(runs):
    """[(length, op char)] -> CIGAR words"""
    return [(n << 4) | OPS.index(op) for n, op in runs]


def sam_model(texts, alphabet, queries, strands, mode, max_edits, win_query, win_text_ids, dist, begin, end, n_cigar, cigar, mapq,
              proper=None, names=None, text_names=None, dense_to_io=None):
    """-> (records: list of bytes, status: list).  queries: the nq = n_reads * strands reads; cigar: rows of 2 max_edits + 1 words"""
    tab = default_table(alphabet) if dense_to_io is None else bytes(dense_to_io)
    dense = np.asarray(alphabet.io_to_dense_table, dtype=np.int64)
    n, stride = len(win_query), 2 * max_edits + 1
    assert len(queries) == n * strands and (mode == SINGLE or n % 2 == 0)
    mapped, status = [], []
    for r in range(n):
        wq = int(win_query[r])
        ok, bad = False, False
        if wq != NONE:
            if not r * strands <= wq < (r + 1) * strands or int(win_text_ids[r]) >= len(texts) or int(n_cigar[r]) > stride:
                bad = True
            elif int(end[r]) != NO_END:
                if sum(int(w) >> 4 for w in cigar[r][:int(n_cigar[r])]) > MAX_RUN_SUM:
                    bad = True
                else:
                    ok = True
        mapped.append(ok)
        status.append(BAD_RECORD if bad else 0)

    def text_name(t):
        return bytes(text_names[t]) if text_names is not None else b"%d" % t

    def symbol(t, y):
        if y >= len(texts[t]):
            return b"?"
        d = int(dense[texts[t][y]])
        return bytes([tab[d if 1 <= d <= 4 else 0]])

    records = []
    for r in range(n):
        m = r ^ 1
        me, mate = mapped[r], mode == PAIRED and mapped[m]
        strand = int(win_query[r]) - r * strands if me else 0
        t, b, e = (int(win_text_ids[r]), int(begin[r]), int(end[r])) if me else (0, 0, 0)
        tm, bm, em = (int(win_text_ids[m]), int(begin[m]), int(end[m])) if mate else (0, 0, 0)
        qname = bytes(names[r]) if names is not None else b"%d" % (r // 2 if mode == PAIRED else r)
        flag = 0
        if mode == PAIRED:
            flag |= 0x1 | (0x80 if r & 1 else 0x40)
            if me and mate and proper is not None and int(proper[r // 2]) != 0:
                flag |= 0x2
            if not mate:
                flag |= 0x8
            if mate and int(win_query[m]) - m * strands == 1:
                flag |= 0x20
        if not me:
            flag |= 0x4
        if me and strand == 1:
            flag |= 0x10
        runs = [(int(w) >> 4, int(w) & 15) for w in cigar[r][:int(n_cigar[r])]] if me else []
        cig = b"".join(b"%d%s" % (ln, (OPS[op] if op <= 8 else "?").encode()) for ln, op in runs) or b"*"
        together = me and mate and t == tm
        rnext = b"*" if not mate else (b"=" if together else text_name(tm))
        tlen = 0
        if together:
            span = max(e, em) - min(b, bm)
            tlen = span if b < bm or (b == bm and r % 2 == 0) else -span
        seq = bytes(queries[int(win_query[r]) if me else r * strands]) or b"*"
        fields = [qname, b"%d" % flag, text_name(t) if me else b"*", b"%d" % (b + 1 if me else 0),
                  b"%d" % (min(int(mapq[r]), 255) if me else 0), cig, rnext, b"%d" % (bm + 1 if mate else 0), b"%d" % tlen, seq, b"*"]
        if me:
            md, y, cnt = b"", b, 0
            for ln, op in runs:
                if ln == 0:
                    continue
                if op == EQ:
                    cnt, y = cnt + ln, y + ln
                elif op == DIFF:
                    for _ in range(ln):
                        md += b"%d" % cnt + symbol(t, y)
                        cnt, y = 0, y + 1
                elif op == DEL:
                    md += b"%d^" % cnt + b"".join(symbol(t, y + i) for i in range(ln))
                    cnt, y = 0, y + ln
            md += b"%d" % cnt
            fields += [b"NM:i:%d" % int(dist[r]), b"MD:Z:" + md]
        records.append(b"\t".join(fields) + b"\n")
    return records, status


def record_bound(max_read_len, max_name_len, max_text_name_len, k):
    """the formula of gdx_sam_record_bound as the header states it"""
    d = len(str(max_read_len + k))
    return (max(max_name_len, 10) + 4 + 2 * max(max_text_name_len, 10) + 10 + 3 + (2 * k + 1) * (d + 1) + 10 + 11 + max(max_read_len, 1)
            + 1 + 15 + (5 + (k + 1) * d + 2 * k) + 12 + 1)


def rebuild_segment(line):
    """text[begin:end] of a mapped record from SEQ, CIGAR and MD alone -> (text id field, begin, segment)"""
    f = line.rstrip(b"\n").split(b"\t")
    seq = b"" if f[9] == b"*" else f[9]
    md = [x for x in f[12:] if x.startswith(b"MD:Z:")][0][5:]
    runs = [] if f[5] == b"*" else [(int(n), op) for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", f[5])]
    tokens = re.findall(rb"\d+|\^[^\d^]+|[^\d^]", md)       # a count, a deletion, a mismatched text symbol
    at = [0]

    def next_token():
        at[0] += 1
        return tokens[at[0] - 1]

    out, x, left = bytearray(), 0, int(next_token())           # left: what the current count still covers
    for n, op in runs:
        if op == b"=":
            assert left >= n
            out += seq[x:x + n]
            x, left = x + n, left - n
        elif op == b"X":
            for _ in range(n):
                assert left == 0
                out += next_token()
                left = int(next_token())
            x += n
        elif op == b"D":
            assert left == 0
            tok = next_token()
            assert tok[:1] == b"^" and len(tok) == n + 1
            out += tok[1:]
            left = int(next_token())
        elif op == b"I":
            x += n
    assert left == 0 and at[0] == len(tokens) and x == len(seq)
    return f[2], int(f[3]) - 1, bytes(out)


def one(texts, reads, rows, **kw):
    """rows: per read (win_query, text id, dist, begin, end, runs, mapq) -> the records as one bytes"""
    k = kw.pop("k", 3)
    cigar = np.zeros((len(rows), 2 * k + 1), dtype=np.uint32)
    for r, row in enumerate(rows):
        w = words(row[5])[:2 * k + 1]                       # (a row that claims more runs than the stride holds keeps its claim)
        cigar[r, :len(w)] = w
    col = lambda i: [row[i] for row in rows]  # noqa: E731
    recs, status = sam_model(texts, A, reads, kw.pop("strands", 1), kw.pop("mode", SINGLE), k, col(0), col(1), col(2), col(3), col(4),
                             [len(row[5]) for row in rows], cigar, col(6), **kw)
    return recs, status


UNMAPPED = (NONE, 0, 4, NO_END, NO_END, [], 255)


def test_the_worked_example_of_single_mode():
    texts = [b"TTACGGATCCAGTTAGC"]
    runs = [(4, "="), (1, "X"), (3, "="), (1, "D"), (3, "="), (1, "I"), (3, "=")]
    recs, status = one(texts, [b"ACGGTTCCGTTCAGC"], [(0, 0, 3, 2, 17, runs, 37)], text_names=[b"chr1"])
    assert recs == [b"0\t0\tchr1\t3\t37\t4=1X3=1D3=1I3=\t*\t0\t0\tACGGTTCCGTTCAGC\t*\tNM:i:3\tMD:Z:4A3^A6\n"] and status == [0]
    assert rebuild_segment(recs[0]) == (b"chr1", 2, texts[0][2:17])


def test_the_md_example_of_the_header():
    texts = [b"GGACGT"]                                  # 2=1D1X2= over ..AC..
    recs, _ = one(texts, [b"GGTGT"], [(0, 0, 2, 0, 6, [(2, "="), (1, "D"), (1, "X"), (2, "=")], 0)])
    assert recs[0].endswith(b"\tMD:Z:2^A0C2\n")


def test_the_worked_example_of_paired_mode():
    text = random_text(np.random.default_rng(1), 400)
    rc = alph.reverse_complement
    # strands = 2: query 2r is read r as given, 2r + 1 its reverse complement; read 1 was sequenced from the reverse strand
    reads = [text[100:108], rc(text[100:108]), rc(text[300:308]), text[300:308]]
    rows = [(0, 0, 0, 100, 108, [(8, "=")], 60), (3, 0, 0, 300, 308, [(8, "=")], 60)]
    recs, _ = one([text], reads, rows, strands=2, mode=PAIRED, proper=[1])
    a, b = (r.split(b"\t") for r in recs)
    assert (a[0], a[1], a[6], a[7], a[8]) == (b"0", b"99", b"=", b"301", b"208")
    assert (b[0], b[1], b[6], b[7], b[8]) == (b"0", b"147", b"=", b"101", b"-208")
    assert a[9] == text[100:108] and b[9] == text[300:308]


def test_hand_written_cases():
    t0, t1 = b"ACGTACGTAC", b"TTTTGGGG"
    hit = lambda wq, t, b, e, runs, q=30, d=0: (wq, t, d, b, e, runs, q)  # noqa: E731
    # an unmapped read, alone and as a mate; its SEQ is the read as given
    recs, status = one([t0], [b"GGG"], [UNMAPPED])
    assert recs == [b"0\t4\t*\t0\t0\t*\t*\t0\t0\tGGG\t*\n"] and status == [0]
    recs, _ = one([t0, t1], [b"ACGT", b"CC"], [hit(0, 0, 0, 4, [(4, "=")]), UNMAPPED], mode=PAIRED, proper=[1])
    assert recs[0] == b"0\t73\t0\t1\t30\t4=\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4\n"         # 1 + 8 + 64: the mate unmapped, not proper
    assert recs[1] == b"0\t133\t*\t0\t0\t*\t0\t1\t0\tCC\t*\n"                               # 1 + 4 + 128; RNEXT is the mate's text
    # mates on different texts: the other's name, no TLEN, never proper
    recs, _ = one([t0, t1], [b"ACGT", b"TTGG"], [hit(0, 0, 0, 4, [(4, "=")]), hit(1, 1, 2, 6, [(4, "=")])], mode=PAIRED, proper=[1],
                  text_names=[b"one", b"two"])
    assert recs[0].split(b"\t")[1:9] == [b"67", b"one", b"1", b"30", b"4=", b"two", b"3", b"0"]
    assert recs[1].split(b"\t")[1:9] == [b"131", b"two", b"3", b"30", b"4=", b"one", b"1", b"0"]
    # equal begins: the even mate has the positive TLEN
    recs, _ = one([t0], [b"ACGT", b"ACGTAC"], [hit(0, 0, 0, 4, [(4, "=")]), hit(1, 0, 0, 6, [(6, "=")])], mode=PAIRED)
    assert [r.split(b"\t")[8] for r in recs] == [b"6", b"-6"]
    # an X directly after a D, and a D directly after an X
    recs, _ = one([b"ACGTAC"], [b"ATAC"], [hit(0, 0, 0, 6, [(1, "="), (2, "D"), (1, "X"), (2, "=")], d=3)])
    assert recs[0].endswith(b"MD:Z:1^CG0T2\n")
    recs, _ = one([b"ACGTAC"], [b"AGAC"], [hit(0, 0, 0, 6, [(1, "="), (1, "X"), (2, "D"), (2, "=")], d=3)])
    assert recs[0].endswith(b"MD:Z:1C0^GT2\n")
    # a CIGAR that walks beyond the text: ? for what is not there
    recs, _ = one([b"ACG"], [b"ACTT"], [hit(0, 0, 0, 4, [(2, "="), (2, "X")], d=2)])
    assert recs[0].endswith(b"MD:Z:2G0?0\n")
    recs, _ = one([b"ACG"], [b"AC"], [hit(0, 0, 1, 5, [(2, "="), (2, "D")], d=2)])
    assert recs[0].endswith(b"MD:Z:2^??0\n")
    # an N of the text; an unknown symbol table entry
    recs, _ = one([b"ANGT"], [b"ACGT"], [hit(0, 0, 0, 4, [(1, "="), (1, "X"), (2, "=")], d=1)])
    assert recs[0].endswith(b"MD:Z:1N2\n")
    recs, _ = one([b"ANGT"], [b"ACGT"], [hit(0, 0, 0, 4, [(1, "="), (1, "X"), (2, "=")], d=1)], dense_to_io=b"nacgt" + b"." * 11)
    assert recs[0].endswith(b"MD:Z:1n2\n")
    # an empty read, mapped (no runs) and unmapped
    recs, _ = one([t0], [b"", b""], [hit(0, 0, 3, 3, []), UNMAPPED])
    assert recs == [b"0\t0\t0\t4\t30\t*\t*\t0\t0\t*\t*\tNM:i:0\tMD:Z:0\n", b"1\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"]
    # mapq 255 and above
    recs, _ = one([t0], [b"ACGT"] * 3, [hit(r, 0, 0, 4, [(4, "=")], q=q) for r, q in enumerate((254, 255, 0xFFFFFFFF))])
    assert [r.split(b"\t")[4] for r in recs] == [b"254", b"255", b"255"]
    # a bad win_query (another read's), a text id out of range, too many runs, runs too long: unmapped and flagged
    rows = [hit(1, 0, 0, 4, [(4, "=")]), hit(1, 5, 0, 4, [(4, "=")]), (2, 0, 0, 0, 4, [(1, "=")] * 8, 30), hit(3, 0, 0, 4, [(MAX_RUN_SUM + 1, "=")]),
            hit(4, 0, 0, 4, [(MAX_RUN_SUM, "=")]), (7, 0, 4, NO_END, NO_END, [], 255)]
    recs, status = one([t0], [b"ACGT"] * 6, rows)
    assert status == [1, 1, 1, 1, 0, 1] and all(r.split(b"\t")[1] == b"4" for i, r in enumerate(recs) if i != 4)
    assert recs[4].split(b"\t")[5] == b"%d=" % MAX_RUN_SUM
    # both strands: strand 1 sets 0x10 and prints the reverse complement, which is the query itself
    recs, _ = one([t0], [b"GTAC", b"GTAC"], [hit(1, 0, 2, 6, [(4, "=")])], strands=2)
    assert recs[0].split(b"\t")[1] == b"16" and recs[0].split(b"\t")[9] == b"GTAC"
    # names
    recs, _ = one([t0], [b"ACGT", b"CC"], [hit(0, 0, 0, 4, [(4, "=")]), UNMAPPED], names=[b"read/1", b""])
    assert recs[0].startswith(b"read/1\t0\t") and recs[1].startswith(b"\t4\t")


def test_the_default_table():
    assert default_table(A)[:6] == b"NACGTN" and default_table(alph.ascii_dna())[:6] == b"?ACGT?"
    assert default_table(alph.ascii_dna_iupac())[:6] == b"?ACGTN"                   # several codes above 4: not known which
    assert default_table(alph.ascii_dna_iupac_as_dna_with_n())[:6] == b"BACGTB"    # one code, its smallest byte


def random_alignments(rng, texts, n, k, lengths):
    """n reads taken from the texts with up to k planted edits -> (reads, cand_query, cand_begin, hits)"""
    reads, hits = [], []
    for i in range(n):
        t = int(rng.integers(0, len(texts)))
        ln = int(lengths[i % len(lengths)])
        at = int(rng.integers(0, max(len(texts[t]) - ln, 0) + 1))
        q = bytearray(texts[t][at:at + ln])
        for _ in range(int(rng.integers(0, k + 1))):
            if not q:
                break
            p, kind = int(rng.integers(0, len(q))), int(rng.integers(0, 3))
            if kind == 0:
                q[p] = b"ACGT"[int(rng.integers(0, 4))]
            elif kind == 1:
                del q[p]
            else:
                q.insert(p, b"ACGT"[int(rng.integers(0, 4))])
        reads.append(bytes(q[:256]))
        hits.append((t, at))
    return reads, np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.array(hits, dtype=np.uint64)


def test_random_alignments_rebuild_their_text_segment():
    rng = np.random.default_rng(2301)
    texts = [random_text(rng, 700, 0.02), random_text(rng, 90, 0.0), random_text(rng, 400, 0.05)]
    k = 6
    reads, cq, cb, hits = random_alignments(rng, texts, 120, k, (0, 1, 5, 30, 64, 65, 150, 256))
    dist, begin, end, n_cigar, cigar = align_model(texts, A, reads, cq, cb, hits, k)
    wq = np.where(end != NO_END, cq, NONE)
    recs, status = sam_model(texts, A, reads, 1, SINGLE, k, wq, hits[:, 0], dist, begin, end, n_cigar, cigar, np.full(len(reads), 60))
    assert not any(status) and (end != NO_END).sum() >= 90     # (a read longer than its text, or on many N, finds nothing)
    longest = max(len(q) for q in reads)
    for r, line in enumerate(recs):
        assert len(line) <= record_bound(longest, 0, 0, k)
        if end[r] == NO_END:
            assert line.split(b"\t")[1] == b"4"
            continue
        name, b, segment = rebuild_segment(line)
        assert int(name) == hits[r, 0] and b == begin[r]
        assert segment == texts[int(name)][b:int(end[r])], (r, line)
        assert int(re.search(rb"NM:i:(\d+)", line).group(1)) == dist[r]


def test_header_library_stub_and_rust_binding_have_the_calls():
    header = open(os.path.join(ROOT, "include", "gdx_experimental.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    from genedex_amd import _lib

    for name in ("gdx_sam_records_many", "gdx_sam_records_many_dev", "gdx_sam_workspace_bytes", "gdx_sam_record_bound"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES and re.search(r"\bfn %s\(" % name, rust), name
    assert "gdx_sam_inputs_t" in header and hasattr(_lib, "SamInputs") and "SamInputs" in rust
    # the argument block of the stub has the header's fields in the header's order
    block = header[header.index("typedef struct gdx_sam_inputs_t {"):header.index("} gdx_sam_inputs_t;")]
    block = re.sub(r"/\*.*?\*/", "", block, flags=re.S)
    fields = re.findall(r"\*?\b([a-z_]+)\s*[,;]", block)
    assert fields == [name for name, _ in _lib.SamInputs._fields_], fields
    assert (_lib.GDX_SAM_SINGLE, _lib.GDX_SAM_PAIRED, _lib.GDX_SAM_BAD_RECORD, _lib.GDX_SAM_MAX_RUN_SUM) == (SINGLE, PAIRED, BAD_RECORD, MAX_RUN_SUM)


def test_the_sam_header_and_writer(tmp_path):
    from genedex_amd import sam

    head = sam.header([b"chr1", "chr2"], [17, 5])
    assert head == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:17\n@SQ\tSN:chr2\tLN:5\n"
    assert sam.header(None, [3]) == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:0\tLN:3\n"
    path = tmp_path / "out.sam"
    body = np.frombuffer(b"0\t4\t*\t0\t0\t*\t*\t0\t0\tGGG\t*\n", dtype=np.uint8)
    assert sam.write(str(path), body, [b"chr1", b"chr2"], [17, 5]) == len(head) + body.size
    assert path.read_bytes() == head + body.tobytes()
