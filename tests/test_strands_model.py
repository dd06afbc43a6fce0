"""Both strands, the part that needs no device: the stock complement table and its two rules, reverse_complement, the
byte counts of gdx_strands_out_bytes, and a numpy model of the expanded batch (all four layouts, both modes) that
tests/test_gpu_strands.py compares gdx_strands_expand_dev with, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from genedex_amd import _lib
from genedex_amd import alphabet as alph

REVERSE, BOTH = _lib.GDX_STRANDS_REVERSE, _lib.GDX_STRANDS_BOTH
DNA_ALPHABETS = ("ascii_dna", "ascii_dna_with_n", "ascii_dna_iupac", "ascii_dna_iupac_as_dna_with_n")
IUPAC = b"ACGTRYKMBVDHSWN"


def out_bytes(total_symbols, packed, mode):
    return int(_lib.load().gdx_strands_out_bytes(int(total_symbols), int(packed), int(mode)))


def packed_bytes(n_symbols):
    return int(_lib.load().gdx_packed_bytes(int(n_symbols)))


def pack_codes(codes, nbytes):
    """2-bit codes -> the packed form of gdx.h: symbol j in bits 2 (j & 3) .. of byte j >> 2; zero padding up to nbytes"""
    codes = np.asarray(codes, dtype=np.uint8)
    padded = np.zeros((codes.size + 3) // 4 * 4, dtype=np.uint8)
    padded[:codes.size] = codes
    q = padded.reshape(-1, 4)
    out = np.zeros(nbytes, dtype=np.uint8)
    out[:q.shape[0]] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
    return out


def unpack_codes(packed, n_symbols):
    b = np.asarray(packed, dtype=np.uint8)[:(n_symbols + 3) // 4]
    return np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)[:n_symbols]


def expand_model(qbuf, qoff, nq, mode, packed=False, uniform_len=0, complement=None):
    """What gdx_strands_expand_dev leaves behind: (the whole output buffer, the output offsets or None).  qbuf: the input
    buffer in its form (IO symbols, or 2-bit codes when packed); qoff: u64[nq + 1] counting symbols, ignored for a uniform
    batch.  Written from the definition: symbols are moved one query at a time."""
    if uniform_len:
        qoff = np.arange(nq + 1, dtype=np.uint64) * np.uint64(uniform_len)
    qoff = np.asarray(qoff, dtype=np.uint64) if nq else np.zeros(1, dtype=np.uint64)
    total = int(qoff[nq])
    if packed:
        sym = unpack_codes(qbuf, total)
        comp = lambda s: s ^ 3  # noqa: E731
    else:
        sym = np.asarray(qbuf, dtype=np.uint8)[:total]
        table = alph.dna_complement_table() if complement is None else np.asarray(complement, dtype=np.uint8)
        comp = lambda s: table[s]  # noqa: E731
    out = np.zeros(mode * total, dtype=np.uint8)
    out_off = np.zeros(2 * nq + 1, dtype=np.uint64)
    base = int(qoff[0])
    for i in range(nq):
        b, e = int(qoff[i]), int(qoff[i + 1])
        rc = comp(sym[b:e][::-1])
        if mode == REVERSE:
            out[b:e] = rc
        else:
            o, ln = 2 * (b - base), e - b
            out[o:o + ln] = sym[b:e]
            out[o + ln:o + 2 * ln] = rc
            out_off[2 * i], out_off[2 * i + 1] = o, o + ln
    out_off[2 * nq] = 2 * (total - base)
    nbytes = out_bytes(total, packed, mode)
    if packed:
        buf = pack_codes(out, nbytes)
    else:
        buf = np.zeros(nbytes, dtype=np.uint8)
        buf[:out.size] = out
    return buf, (out_off if mode == BOTH and not uniform_len else None)


def host_batches(qs, complement=None):
    """(reverse complements, both strands interleaved) of a list of reads, made on the host"""
    rc = [alph.reverse_complement(q, complement) for q in qs]
    return rc, [x for pair in zip(qs, rc) for x in pair]


def join(qs):
    """list of reads -> (padded IO buffer, u64 offsets)"""
    off = np.zeros(len(qs) + 1, dtype=np.uint64)
    np.cumsum([len(q) for q in qs], out=off[1:])
    buf = np.zeros((int(off[-1]) + 8 + 7) // 8 * 8, dtype=np.uint8)
    buf[:int(off[-1])] = np.frombuffer(b"".join(qs), dtype=np.uint8)
    return buf, off


def random_reads(rng, n, lo, hi, symbols=b"ACGT"):
    return [bytes(symbols[k] for k in rng.integers(0, len(symbols), int(rng.integers(lo, hi + 1)))) for _ in range(n)]


# ------------------------------------------------------------------------------------------------

def test_the_stock_table():
    lib = _lib.load()
    t = np.zeros(256, dtype=np.uint8)
    lib.gdx_dna_complement_table(t.ctypes.data_as(_lib.u8p))
    assert np.array_equal(t, alph.dna_complement_table())
    assert np.array_equal(t[t], np.arange(256, dtype=np.uint8)), "not an involution"
    pairs = dict(zip(IUPAC, b"TGCAYRMKVBHDSWN"))
    for c in range(256):
        if c in pairs:
            assert t[c] == pairs[c] and t[c + 32] == pairs[c] + 32, c
        elif c - 32 not in pairs:
            assert t[c] == c, c
    for c in IUPAC:
        assert chr(t[c]).isupper() and chr(t[c + 32]).islower()


def keeps_validity(io_to_dense, comp):
    return all((io_to_dense[c] == 0) == (io_to_dense[comp[c]] == 0) for c in range(256))


def packed_rule(io_to_dense, comp):
    return all(io_to_dense[comp[c]] == 5 - io_to_dense[c] for c in range(256) if 1 <= io_to_dense[c] <= 4)


def test_the_stock_table_against_the_stock_alphabets():
    t = alph.dna_complement_table()
    for name in DNA_ALPHABETS:
        d = getattr(alph, name)().io_to_dense_table
        assert keeps_validity(d, t), name
        assert packed_rule(d, t), name
    assert not keeps_validity(alph.ascii_amino_acid().io_to_dense_table, t)  # V is valid, B is not


def test_reverse_complement():
    rng = np.random.default_rng(1)
    t = alph.dna_complement_table()
    for m in range(71):
        q = bytes(rng.integers(0, 256, m, dtype=np.uint8)) if m % 2 else random_reads(rng, 1, m, m, b"ACGTNacgtnRYKMBVDHSW")[0]
        want = bytes(int(t[q[m - 1 - j]]) for j in range(m))
        assert alph.reverse_complement(q) == want
        assert alph.reverse_complement(alph.reverse_complement(q)) == q
    swap = np.arange(256, dtype=np.uint8)
    swap[ord("A")], swap[ord("C")] = ord("C"), ord("A")
    assert alph.reverse_complement(b"AACG", swap) == b"GACC"


def test_out_bytes():
    for total in (0, 1, 7, 8, 9, 63, 64, 65, 1000, 12345):
        for mode in (REVERSE, BOTH):
            assert out_bytes(total, 0, mode) == (mode * total + 7) // 8 * 8 + 8
            assert out_bytes(total, 1, mode) == packed_bytes(mode * total)
    assert out_bytes(0, 0, BOTH) == 8 and out_bytes(0, 1, BOTH) == packed_bytes(0)


def _cases(rng):
    yield random_reads(rng, 40, 0, 70), 0
    yield random_reads(rng, 30, 0, 3), 0          # several reads in one packed word and in one 8-byte word
    yield random_reads(rng, 1, 5000, 5000), 0
    for ulen in (1, 3, 16, 17, 49, 50, 51):
        yield random_reads(rng, 33, ulen, ulen), ulen


@pytest.mark.parametrize("mode", (REVERSE, BOTH))
def test_the_model_against_the_definition_and_the_packer(mode):
    lib = _lib.load()
    rng = np.random.default_rng(7)
    dense = alph.ascii_dna().io_to_dense_table
    for qs, ulen in _cases(rng):
        nq = len(qs)
        buf, off = join(qs)
        rc, both = host_batches(qs)
        want_qs = rc if mode == REVERSE else both
        got, got_off = expand_model(buf, off, nq, mode, uniform_len=ulen)
        # the definition, symbol by symbol
        want_buf, want_off = join(want_qs)
        assert got.size == out_bytes(int(off[-1]), 0, mode)
        assert bytes(got[:int(want_off[-1])]) == bytes(want_buf[:int(want_off[-1])]) and not got[int(want_off[-1]):].any()
        for i, q in enumerate(want_qs):
            for j in range(len(q)):
                assert got[int(want_off[i]) + j] == q[j]
        if mode == BOTH and not ulen:
            assert np.array_equal(got_off, want_off)
        else:
            assert got_off is None
        # packing the model's plain output gives the model's packed output
        packed_in = pack_codes(dense[buf[:int(off[-1])]] - 1, packed_bytes(int(off[-1])))
        got_p, got_p_off = expand_model(packed_in, off, nq, mode, packed=True, uniform_len=ulen)
        via_packer = np.zeros(packed_bytes(int(want_off[-1])), dtype=np.uint8)
        n_exc = C.c_uint64(0)
        _lib.check(lib.gdx_pack_queries_table(dense.ctypes.data_as(_lib.u8p), got.ctypes.data_as(_lib.u8p),
                                              want_off.ctypes.data_as(_lib.u64p), len(want_qs), via_packer.ctypes.data_as(_lib.u8p),
                                              None, 0, C.byref(n_exc)))
        assert n_exc.value == 0
        assert got_p.size == out_bytes(int(off[-1]), 1, mode) == via_packer.size
        assert np.array_equal(got_p, via_packer)
        if got_off is not None:
            assert np.array_equal(got_p_off, got_off)


def test_the_model_on_a_view_that_starts_inside_its_buffer():
    rng = np.random.default_rng(9)
    qs = random_reads(rng, 12, 0, 40)
    buf, off = join(qs)
    view = off[3:]                                 # qoff[0] > 0
    rc, both = host_batches(qs[3:])
    got, _ = expand_model(buf, view, len(view) - 1, REVERSE)
    assert not got[:int(view[0])].any() and bytes(got[int(view[0]):int(view[-1])]) == b"".join(rc)
    got, got_off = expand_model(buf, view, len(view) - 1, BOTH)
    want_buf, want_off = join(both)
    assert np.array_equal(got_off, want_off) and bytes(got[:int(want_off[-1])]) == b"".join(both)
    assert not got[int(want_off[-1]):].any()
