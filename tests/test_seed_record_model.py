"""The plain model of the seed table's repeat records (seed_record_model.py) against the CPU oracle, on the crafted texts:
the GPU tests of the records (test_gpu_seed_records.py) trust it, so it is checked here first, without a GPU."""
import numpy as np
import pytest

from genedex_amd import alphabet as alph
from oracle.oracle import OracleIndex
from seed_record_model import CONTEXT, SEED_ZONE, RecordModel, crafted_reads, crafted_texts, expand_record


def oracle_for(texts):
    a = alph.ascii_dna_with_n()
    return OracleIndex.build(texts, a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(), sa_rate=4,
                             lookup_depth=0, width=32)


@pytest.fixture(scope="module")
def crafted():
    texts, fams = crafted_texts()
    return texts, fams, oracle_for(texts)


@pytest.mark.parametrize("k", [16, 11, 24])
def test_model_hits_are_the_oracles(crafted, k):
    """Every read the model says a record decides: the record expands to the oracle's hits, in the oracle's order."""
    texts, fams, o = crafted
    model = RecordModel(texts, k, o)
    qs = crafted_reads(texts, fams, k)
    co, ct, cp = o.locate_many(qs)
    kinds = {}
    masks = {2: set(), 3: set(), 4: set()}
    n_vs = set()
    for i, q in enumerate(qs):
        got = model.read(q)
        if got is None:
            continue
        kind, mask, rec, hits = got
        kinds[kind] = kinds.get(kind, 0) + 1
        lo, hi, _, pos = model.kmers[model.dense_of(q[len(q) - k:])]
        masks[hi - lo].add(mask)
        n_vs.add(len(q) - k)
        assert expand_record(model, rec) == hits, q
        want = list(zip(ct[co[i]:co[i + 1]].tolist(), cp[co[i]:co[i + 1]].tolist()))
        assert [model.text_pos(h) for h in hits] == want, q
        assert rec[1] - rec[0] == len(want) or (kind == "two" and (rec[1] - rec[0]) & 0xFFFFFFFF == 2)
    # the edges are there on purpose, not by chance
    assert all(kinds.get(kd, 0) >= 20 for kd in ("none", "one", "two", "masked3", "masked4")), kinds
    assert masks[2] == set(range(4)) and masks[3] == set(range(8)) and masks[4] == set(range(16)), masks
    assert {1, 2, 16, 31, 32} <= n_vs and max(n_vs) == CONTEXT
    assert model.pair_records > 0 and model.quad_records > 0


def test_model_records_are_the_definition(crafted):
    """Pair / quad records counted straight from the texts (the k-mers on two / three or four rows whose every occurrence has
    32 symbols A C G T of its own text in front) are the model's; the edges of the crafted texts get a record or none as
    they should."""
    texts, fams, o = crafted
    k = 16
    model = RecordModel(texts, k, o)
    occ = {}
    for t, txt in enumerate(texts):
        for i in range(len(txt) - k + 1):
            w = txt[i:i + k]
            if b"N" not in w:
                occ.setdefault(w, []).append((t, i))
    whole = lambda lst: all(i >= CONTEXT and b"N" not in texts[t][i - CONTEXT:i] for t, i in lst)  # noqa: E731
    assert model.pair_records == sum(1 for v in occ.values() if len(v) == 2 and whole(v))
    assert model.quad_records == sum(1 for v in occ.values() if len(v) in (3, 4) and whole(v))
    assert len(model.kmers) == len(occ)
    kinds = [model.kmers[model.dense_of(f.zone[:k])][2] for f in fams]
    rows = [model.kmers[model.dense_of(f.zone[:k])][1] - model.kmers[model.dense_of(f.zone[:k])][0] for f in fams]
    assert rows == [f.copies for f in fams]
    assert all(kd is None for kd, f in zip(kinds, fams) if f.copies == 5)
    # (the families after the mask families: 2/3/4/5/5 copies, then text starts at 31, 32, 33, then N at 0 / 31 / -33)
    tail = kinds[-18:]
    assert tail[0:3] == [None] * 3                      # a copy's seed 31 symbols after its text's start: not whole
    assert tail[3:6] == ["pair", "quad", "quad"] and tail[6:9] == ["pair", "quad", "quad"]  # 32, 33
    assert tail[9:15] == [None] * 6                     # an N at either end of a context
    assert tail[15:18] == ["pair", "quad", "quad"]      # ... and one symbol in front of it
    assert SEED_ZONE >= 24


def test_expand_record_reads_the_masked_form(crafted):
    """A masked record's hits are SA[first row + j] - symbols for the set bits j, in row order."""
    texts, _, o = crafted
    model = RecordModel(texts, 16, o)
    quad = next(v for v in model.kmers.values() if v[2] == "quad" and v[1] - v[0] == 4)
    lo, _, _, pos = quad
    rec = (lo, lo + 3, 0b1101, 5 | (1 << 23))
    assert expand_record(model, rec) == [pos[0] - 5, pos[2] - 5, pos[3] - 5]
    assert expand_record(model, (7, 9, 3, 1 << 22)) == [3, 7]
    assert expand_record(model, (0, 0, 0xFFFFFFFF, 0)) == []
    assert np.all(model.sa[lo:lo + 4] == np.array(pos))
