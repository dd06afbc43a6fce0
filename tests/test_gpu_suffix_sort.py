"""The suffix sorter (build_sa.hip) and the 64-bit engine's (wide.hip, wide_suffix_array) at their borders: chunk borders of the
partition passes, every key width, ties that end on the border of the first key, second keys that fall on the last symbol, the
end of the string and beyond, the sentinel bucket, and lists long enough for the second sweep of the grid-stride kernels.

Every index is built at sampling rate 1 and lookup depth 0, so export_sa_samples() IS the suffix array, in a plain shape (no pair
lines, jump table, top table, seed table, text units or inverse suffix array): the sorter and the BWT pass are what runs.  Every
case is built three times -- 32-bit engine from host texts, 32-bit engine from a text resident on the device, 64-bit engine forced
onto the small input (where it takes the alphabet: up to 7 symbols) -- and checked layer by layer against the plain model of
suffix_array_model.py: the linear-time check of the array, brute force up to 20 000 symbols, the BWT, sentinels / borders /
counts (against the CPU oracle as well up to 300 000 symbols), then what the sorter reports about its own work
(gdx_index_build_stats: initial order, pending suffixes after the key sort, rounds).  The 64-bit engine exports no suffix array and
keeps no build statistics: it is checked through export_bwt() alone, which must equal the 32-bit engine's byte for byte.

export_sentinel_indices() holds the sentinels' positions in the TEXT (construction/mod.rs:266-273); the rows of the BWT that hold
a sentinel are the keys of export_borders(), their suffix-array values its values.  Both are checked.

All equalities are exact."""
import numpy as np
import pytest

import suffix_array_model as model
from genedex_amd import alphabet as alph
from oracle.oracle import OracleIndex, pack_queries

pytestmark = pytest.mark.gpu

PLAIN = dict(pair_lines=False, jump_entry_bytes=0, top_table_depth=0, seed_symbols=0, text_units=False,
             inverse_suffix_array=False)
ORACLE_LIMIT = 300_000

DNA = alph.ascii_dna()                                   # sigma 5, 3 bits, k0 21
DNA_N = alph.ascii_dna_with_n()                          # sigma 6
AC = alph.Alphabet.from_io_symbols(b"AC")                # sigma 3, 2 bits, k0 32: the key fills all 64 bits
ONLY_A = alph.Alphabet.from_io_symbols(b"A")             # sigma 2, 2 bits, k0 32
H0 = {"dna": 22, "ac": 33}
ALPHABETS = {"dna": DNA, "ac": AC}


def random_text(rng, symbols: bytes, length: int) -> bytes:
    return np.frombuffer(symbols, dtype=np.uint8)[rng.integers(0, len(symbols), length)].tobytes()


# ---- the three forms of an index -------------------------------------------------------------------------------------------------

def build_host(texts, a, shape):
    from genedex_amd import FmIndexConfig

    return (FmIndexConfig("u32").suffix_array_sampling_rate(1).lookup_table_depth(0).acceleration_structures(**shape)
            .construct_index(texts, a))


def build_from_device_text(texts, a, shape):
    import torch

    from genedex_amd.device import build_index_from_device_text
    from genedex_amd.index import build_options

    io = np.frombuffer(b"".join(texts), dtype=np.uint8)
    d_io = torch.zeros(max(io.size, 1), dtype=torch.uint8, device="cuda")
    if io.size:
        d_io[: io.size] = torch.from_numpy(io.copy()).cuda()
    return build_index_from_device_text(d_io, [len(t) for t in texts], a, sa_rate=1, lookup_depth=0, index_storage="u32",
                                        options=build_options(**shape))


def build_wide(texts, a):
    """the 64-bit engine forced onto a small input, as test_wide_index_equals_oracle_i64 does"""
    from genedex_amd import FmIndexConfig, _lib

    lib = _lib.load()
    lib.gdx_debug_force_wide(1)
    try:
        g = FmIndexConfig("i64").suffix_array_sampling_rate(1).construct_index(texts, a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert g.info.index_width == 64
    return g


def check_case(label, texts, a, max_lcp=None, lcp_cap=None, default_shape=False):
    """All layers of one case, in the order that names the layer of the first failure.  max_lcp: known from the construction of a
    text too long for Kasai's loop; lcp_cap: such a text with short ties (the vectorised LCP up to that cap)."""
    texts = [bytes(t) for t in texts]
    sigma = a.num_dense_symbols()
    dense = model.dense_concat(texts, a)
    n = dense.size

    g = build_host(texts, a, PLAIN)
    assert g.total_text_len() == n and g.num_texts() == len(texts)
    sa = g.export_sa_samples()
    model.check_suffix_array(dense, sa)                                             # 1. the array
    if n <= model.BRUTE_LIMIT:
        assert sa.tolist() == model.brute_suffix_array(dense).tolist()              # 2. brute force
    bwt = g.export_bwt()
    want_bwt = model.bwt_from_sa(dense, sa)
    assert bwt.tobytes() == want_bwt.tobytes()                                      # 3. the BWT
    rows = np.flatnonzero(want_bwt == 0)                                            # 4. sentinels, borders, counts
    keys, vals = g.export_borders()
    assert g.export_sentinel_indices().tolist() == np.flatnonzero(dense == 0).tolist()
    assert keys.tolist() == rows.tolist() and vals.tolist() == sa[rows].tolist()
    count = np.zeros(sigma + 1, dtype=np.uint64)
    count[1:] = np.cumsum(np.bincount(dense, minlength=sigma))
    assert g.export_count().tolist() == count.tolist()
    if n <= ORACLE_LIMIT:
        c = OracleIndex.build(texts, a.io_to_dense_table, sigma, a.num_searchable_dense_symbols(), sa_rate=1, lookup_depth=0,
                              width=32)
        assert g.export_sentinel_indices().tolist() == c.sentinel_indices.tolist()
        assert keys.tolist() == c.border_keys.tolist() and vals.tolist() == c.border_vals.tolist()
        assert g.export_count().tolist() == c.count_array.tolist()
        assert bwt.tobytes() == c.bwt.tobytes() and sa.tolist() == c.sa_samples.tolist()
    if max_lcp is None:
        max_lcp = model.max_lcp_capped(dense, sa, lcp_cap) if lcp_cap else model.max_lcp_kasai(dense, sa)
        assert lcp_cap is None or max_lcp < lcp_cap
    want = dict(sa_initial_order=model.initial_order(sigma), sa_pending_after_sort=model.pending_after_key_sort(dense, sigma),
                sa_rounds=model.rounds_for_max_lcp(max_lcp, sigma))
    stats = g.build_stats()
    got = {k: int(stats[k]) for k in want}
    print(f"suffix sort {label}: n {n} sigma {sigma} order {got['sa_initial_order']} pending {got['sa_pending_after_sort']} "
          f"rounds {got['sa_rounds']}")
    assert got["sa_initial_order"] == want["sa_initial_order"]                      # 5. what the sorter reports
    assert got["sa_pending_after_sort"] == want["sa_pending_after_sort"]
    assert got["sa_rounds"] == want["sa_rounds"]
    del g

    d = build_from_device_text(texts, a, PLAIN)                                     # the same from a device-resident text
    assert d.export_sa_samples().tobytes() == sa.tobytes()
    assert d.export_bwt().tobytes() == bwt.tobytes()
    assert {k: int(v) for k, v in d.build_stats().items() if k in want} == want
    del d
    if sigma <= 8:                                                                  # the 64-bit engine: BWT only (see above)
        w = build_wide(texts, a)
        assert w.total_text_len() == n and w.export_bwt().tobytes() == bwt.tobytes()
        del w
    if default_shape:  # the library's default shape: the extra structures do not disturb the arrays
        f = build_host(texts, a, {})
        assert f.export_sa_samples().tobytes() == sa.tobytes() and f.export_bwt().tobytes() == bwt.tobytes()
        assert {k: int(v) for k, v in f.build_stats().items() if k in want} == want
    return got


# ---- a. chunk borders of the partition passes (4096 positions per chunk) ----------------------------------------------------------

@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("total", [4095, 4096, 4097, 8191, 8192, 8193])
def test_chunk_borders(total, split):
    """One DNA text whose length with its sentinel is `total`; the same total over three texts, one of them empty."""
    rng = np.random.default_rng(total)
    if split:
        body = random_text(rng, b"ACGT", total - 3)
        cut = int(rng.integers(1, total - 4))
        texts = [body[:cut], b"", body[cut:]]
    else:
        texts = [random_text(rng, b"ACGT", total - 1)]
    assert sum(len(t) + 1 for t in texts) == total
    check_case(f"a/{total}/{'three texts' if split else 'one text'}", texts, DNA, default_shape=(total == 4097 and not split))


# ---- b. key width by alphabet size ---------------------------------------------------------------------------------------------

KEY_WIDTHS = {  # symbols: (sigma, sym_bits, k0)
    1: (2, 2, 32), 2: (3, 2, 32), 3: (4, 3, 21), 7: (8, 4, 16), 15: (16, 5, 12), 20: (21, 5, 12), 255: (256, 9, 7)}


@pytest.mark.parametrize("n_symbols", list(KEY_WIDTHS))
def test_key_width(n_symbols):
    """3000 random symbols per alphabet size (one symbol: A^3000); 255 symbols is the largest alphabet there is."""
    sigma, sym_bits, k0 = KEY_WIDTHS[n_symbols]
    symbols = {20: b"ACDEFGHIKLMNPQRSTVWY", 255: bytes(range(255))}.get(n_symbols, b"ACGTNRYKMSWBDHV"[:n_symbols])
    a = alph.Alphabet.from_io_symbols(symbols)
    assert a.num_dense_symbols() == sigma and model.initial_order(sigma) == 1 + k0 and k0 == min(32, 64 // sym_bits)
    rng = np.random.default_rng(n_symbols)
    got = check_case(f"b/{n_symbols} symbols", [random_text(rng, symbols, 3000)], a)
    assert got["sa_initial_order"] == 1 + k0


def test_key_width_with_absent_symbols():
    """DNA with N whose texts hold A, T and N only: the dense symbols in between are in the alphabet and not in the text"""
    rng = np.random.default_rng(77)
    texts = [random_text(rng, b"ATN", 3000), b"", random_text(rng, b"AT", 500), b"N" * 40]
    check_case("b/absent symbols", texts, DNA_N, default_shape=True)


# ---- c. ties that end on the border of the first key; second keys on n - 1, n, n + 1 ---------------------------------------

PERIODS = {"h0-1": lambda h: h - 1, "h0": lambda h: h, "h0+1": lambda h: h + 1, "2h0-1": lambda h: 2 * h - 1,
           "2h0": lambda h: 2 * h, "2h0+1": lambda h: 2 * h + 1}


@pytest.mark.parametrize("whole", [True, False])
@pytest.mark.parametrize("period", list(PERIODS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_repeat_periods_on_the_key_border(alphabet, period, whole):
    """A random unit of p symbols repeated to about 3000, ending on a whole period or cut in the middle of one"""
    h0 = H0[alphabet]
    p = PERIODS[period](h0)
    rng = np.random.default_rng(1000 * h0 + p)
    unit = random_text(rng, b"ACGT" if alphabet == "dna" else b"AC", p)
    length = (3000 // p) * p if whole else (3000 // p) * p + p // 2 + 1
    check_case(f"c/{alphabet}/period {p}/{'whole' if whole else 'cut'}", [model.repeat_to(unit, length)], ALPHABETS[alphabet],
               default_shape=(alphabet == "dna" and period == "h0" and whole))


RUNS = dict(PERIODS)
RUNS.update({"4h0": lambda h: 4 * h, "128h0-1": lambda h: 128 * h - 1, "128h0": lambda h: 128 * h, "128h0+1": lambda h: 128 * h + 1})


@pytest.mark.parametrize("m", list(RUNS))
@pytest.mark.parametrize("alphabet", ["dna", "ac", "a"])
def test_runs_of_one_symbol(alphabet, m):
    """A^m: i + h falls on n - 1, n and n + 1 in the first, the second and the eighth round.  By hand (test_suffix_array_model):
    m + 1 - h0 suffixes pending where that is two or more, and the rounds r with h0 * 2^(r-1) <= m - 1 < h0 * 2^r."""
    a = ONLY_A if alphabet == "a" else ALPHABETS[alphabet]
    h0 = 33 if alphabet == "a" else H0[alphabet]
    length = RUNS[m](h0)
    got = check_case(f"c/{alphabet}/A^{length}", [b"A" * length], a)
    shared = length + 1 - h0
    assert got["sa_pending_after_sort"] == (shared if shared >= 2 else 0)
    rounds = got["sa_rounds"]
    assert rounds == 0 if length <= h0 else h0 * 2 ** (rounds - 1) <= length - 1 < h0 * 2 ** rounds


# ---- d. deep ties with structure ---------------------------------------------------------------------------------------------------

def structured_texts(name):
    if name == "fibonacci":
        return [model.bits_to_text(model.fibonacci_bits(10946), b"AC")]
    if name == "thue-morse":
        return [model.bits_to_text(model.thue_morse_bits(8192), b"AC")]
    if name == "de bruijn":
        return [model.bits_to_text(model.de_bruijn_bits(13), b"AC")]
    return [b"AC" * 2000, b"CA" * 2000, b"AC" * 1999 + b"A"]


@pytest.mark.parametrize("name", ["fibonacci", "thue-morse", "de bruijn", "ac runs"])
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_deep_ties_with_structure(alphabet, name):
    check_case(f"d/{alphabet}/{name}", structured_texts(name), ALPHABETS[alphabet], default_shape=(alphabet == "dna" and name == "ac runs"))


# ---- e. the sentinel bucket --------------------------------------------------------------------------------------------------------

def sentinel_texts(name):
    rng = np.random.default_rng(55)
    if name == "5000 empty":
        return [b""] * 5000
    if name == "3000 empty and a few":
        texts = [b""] * 3000
        for at in rng.choice(3000, 90, replace=False).tolist():
            texts[at] = [b"A", b"C", b"AA"][at % 3]
        return texts
    return [b"ACGT"[i:i + 1] for i in rng.integers(0, 4, 1000).tolist()]


@pytest.mark.parametrize("name", ["5000 empty", "3000 empty and a few", "1000 of one symbol"])
def test_sentinel_bucket(name):
    check_case(f"e/{name}", sentinel_texts(name), DNA, default_shape=(name == "3000 empty and a few"))


# ---- f. second sweep of the round kernels: more than 1 048 576 pending suffixes ------------------------------------------------------

def test_second_sweep_of_the_rounds_repeat():
    """A random DNA unit of 1009 symbols repeated to 1 200 000, one text.  Suffixes a multiple of 1009 apart agree to the end of
    the text, so max LCP = 1 200 000 - 1009, and every suffix that starts at 0 .. 1 200 000 - 22 shares its window of 22 symbols
    with the one a period away: 1 199 979 pending, above the 4096 * 256 lanes of one sweep.  No brute force, no oracle: the
    linear-time check is exact."""
    rng = np.random.default_rng(1009)
    length = 1_200_000
    text = model.repeat_to(random_text(rng, b"ACGT", 1009), length)
    got = check_case("f/unit 1009", [text], DNA, max_lcp=length - 1009)
    assert got["sa_pending_after_sort"] == length - 22 + 1 > 4096 * 256 and got["sa_rounds"] == 16


def test_second_sweep_of_the_rounds_run():
    """A^1 200 000: 1 199 979 pending (test_runs_of_one_symbol), max LCP = m - 1"""
    m = 1_200_000
    got = check_case("f/A^1200000", [b"A" * m], DNA, max_lcp=m - 1)
    assert got["sa_pending_after_sort"] == m + 1 - 22 > 4096 * 256 and got["sa_rounds"] == 16


# ---- g. second sweep of the bucket kernels: first-symbol buckets above 1 048 576 ---------------------------------------------------

def test_second_sweep_of_the_bucket_kernels():
    """2 300 000 i.i.d. symbols of a 2-symbol alphabet: both buckets hold more than 4096 * 256 suffixes, the key takes 32 symbols
    in 64 bits, and a few hundred suffixes stay pending (one sort of the 33-symbol windows in numpy says how many)."""
    rng = np.random.default_rng(23)
    text = random_text(rng, b"AC", 2_300_000)
    assert min(text.count(b"A"), text.count(b"C")) > 4096 * 256
    got = check_case("g/2300000 of AC", [text], AC, lcp_cap=33 * 64)
    assert 0 < got["sa_pending_after_sort"] < 10_000


# ---- h. the per-part sorter of a partitioned index ----------------------------------------------------------------------------------

def test_partitioned_index_on_the_repeat_texts():
    """The repeat texts of group c (periods around the key border, whole and cut) as one collection, cut at text borders into at
    least three parts: hit sets and counts of 200 substrings equal those of the single index, whose suffix array is checked."""
    from genedex_amd import PartitionedFmIndex
    from genedex_amd.index import build_options

    rng = np.random.default_rng(8)
    texts = []
    for p in (21, 22, 23, 43, 44, 45):
        unit = random_text(rng, b"ACGT", p)
        texts += [model.repeat_to(unit, (3000 // p) * p), model.repeat_to(unit, (3000 // p) * p + p // 2 + 1)]
    check_case("h/single index", texts, DNA)
    one = build_host(texts, DNA, PLAIN)
    parts = PartitionedFmIndex.construct(texts, DNA, sa_rate=1, lookup_depth=0, max_part_symbols=9100, options=build_options(**PLAIN))
    assert parts.num_parts >= 3 and parts.total_text_len() == one.total_text_len()
    qs = []
    for _ in range(200):
        t = texts[int(rng.integers(0, len(texts)))]
        at = int(rng.integers(0, len(t)))
        qs.append(t[at:at + int(rng.integers(1, 120))])
    qbuf, qoff = pack_queries(qs)
    off1, t1, p1, _ = one.locate_raw(qbuf, qoff)
    offp, tp, pp, _ = parts.locate_raw(qbuf, qoff)
    assert parts.count_raw(qbuf, qoff)[0].tolist() == np.diff(off1).tolist() == np.diff(offp).tolist()
    assert int(off1[-1]) > 10 * len(qs)
    for q in range(len(qs)):
        a, b = int(off1[q]), int(off1[q + 1])
        assert sorted(zip(t1[a:b].tolist(), p1[a:b].tolist())) == sorted(zip(tp[a:b].tolist(), pp[a:b].tolist())), q
