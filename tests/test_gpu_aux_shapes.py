"""Which auxiliary structures an index gets (aux_plan.hpp decides, FmIndex::build_aux builds): one DNA collection and one
binary-alphabet text built under every kind of option set and every environment override of the aux build, each compared with
tests/golden/aux_shapes.json -- the shapes the library built before the decision moved into aux_plan.hpp, recorded on an
MI355X -- in the fields that depend neither on the device's free memory nor on the order of atomics.  Every index also
answers 200 mixed queries exactly as the oracle does."""
import json
import os

import numpy as np
import pytest

from genedex_amd import _lib, alphabet as alph
from oracle.oracle import pack_queries
from test_gpu_parity import cpu_index, gpu_index, mixed_queries

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aux_shapes.json")
REFUSED = "seed_symbols = 12 needs a seed table of at least"

# name -> (build options, environment override); the three jump / top overrides act on options that are not the default
# shape's (which has no jump table and reads them nowhere)
CASES = {
    "defaults": ({}, {}),
    "budget_1": (dict(aux_budget_bytes=1), {}),
    "budget_300k": (dict(aux_budget_bytes=300_000), {}),
    "jump32_top8": (dict(jump_entry_bytes=32, top_table_depth=8), {}),
    "jump16_top2": (dict(jump_entry_bytes=16, top_table_depth=2), {}),
    "jump8_top4": (dict(jump_entry_bytes=8, top_table_depth=4), {}),
    "no_pair_lines": (dict(pair_lines=False), {}),
    "seed_auto_load40": (dict(seed_symbols=True, seed_load_percent=40), {}),
    "seed12_load40": (dict(seed_symbols=12, seed_load_percent=40), {}),
    "text_units_only": (dict(text_units=True), {}),
    "full_sa_only": (dict(full_suffix_array=True), {}),
    "inverse_sa_only": (dict(inverse_suffix_array=True), {}),
    "seed12_budget_1000": (dict(seed_symbols=12, aux_budget_bytes=1000), {}),
    "reference_layout": (dict(reference_table_layout="condensed64"), {}),
    "env_no_pair_lines": ({}, {"GDX_NO_PAIR_LINES": "1"}),
    "env_default_shape_tables": ({}, {"GDX_DEFAULT_SHAPE": "tables"}),
    "env_aux_budget_gb": ({}, {"GDX_AUX_BUDGET_GB": "0.0003"}),
    "env_jump_bytes": (dict(text_units=False), {"GDX_JUMP_BYTES": "16"}),
    "env_no_jump_table": (dict(text_units=False), {"GDX_NO_JUMP_TABLE": "1"}),
    "env_top_depth": (dict(text_units=False), {"GDX_TOP_DEPTH": "4"}),
}
# one handle: the default shape, explicit tables, the default shape again
REBUILD_STEPS = [dict(jump_entry_bytes=32, top_table_depth=8), {}]


class Workload:
    """a collection, its oracle index, 200 queries and the oracle's answers to them (computed once)"""

    def __init__(self, alphabet, texts, queries):
        self.alphabet, self.texts, self.queries = alphabet, texts, queries
        self.qbuf, self.qoff = pack_queries(queries)
        cpu = cpu_index(texts, alphabet)
        self.intervals = tuple(x.tolist() for x in cpu.cursors_for_many(self.qbuf, self.qoff))
        self.hits = tuple(x.tolist() for x in cpu.locate_many(queries))

    def check_answers(self, index):
        s, e, status = index.cursors_raw(self.qbuf, self.qoff)
        assert not status.any() and (s.tolist(), e.tolist()) == self.intervals
        off, t, p, _ = index.locate_raw(self.qbuf, self.qoff)
        assert (off.tolist(), t.tolist(), p.tolist()) == self.hits


def make_workloads():
    rng = np.random.default_rng(2024)
    dna = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, ln)) for ln in (9000, 7001, 3998)]
    dna[1] = dna[1][:5000] + dna[0][100:1500] + dna[1][6400:]  # a 1400-symbol repeat: two-copy k-mers for the seed table
    binary = [bytes(b"01"[i] for i in rng.integers(0, 2, 20_011))]
    binary_queries = mixed_queries(rng, binary, 150, 0, 70) + [bytes(b"01"[i] for i in rng.integers(0, 2, int(ln)))
                                                               for ln in rng.integers(0, 40, 50)]
    return {"dna": Workload(alph.ascii_dna_with_n(), dna, mixed_queries(rng, dna, 140, 60, 70)),
            "binary": Workload(alph.Alphabet.from_io_symbols(b"01"), binary, binary_queries)}


def shape_of(index, with_budget):
    """what the golden file holds of an index"""
    from genedex_amd.device import DeviceEngine

    aux, info = index.aux(), DeviceEngine(index).aux_info()
    seed = info["seed"]
    shape = {"default_shape": info["default_shape"],
             "wanted_jump_entry_bytes": aux["wanted_jump_entry_bytes"], "wanted_top_table_depth": aux["wanted_top_table_depth"],
             "jump_entry_bytes": info["jump_entry_bytes"], "top_table_depth": info["top_table_depth"],
             "seed": {k: seed[k] for k in ("k", "buckets", "single_entries", "interval_entries", "pair_records", "quad_records")},
             "pair_lines": info["pair_lines"], "text_units": info["text_units"], "full_suffix_array": info["full_suffix_array"],
             "inverse_suffix_array": info["inverse_suffix_array"]}
    assert (aux["jump_entry_bytes"], aux["top_table_depth"]) == (shape["jump_entry_bytes"], shape["top_table_depth"])
    if with_budget:
        shape["aux_budget_bytes"] = aux["aux_budget_bytes"]
    return shape


def observe_case(name, work, setenv, delenv):
    """builds `work` under CASES[name]: the shape (or the refusal's message), with the queries answered"""
    options, env = CASES[name]
    for var, value in env.items():
        setenv(var, value)
    try:
        index = gpu_index(work.texts, work.alphabet, **options)
    except _lib.GdxError as e:
        return {"refused": e.status, "message": str(e)}
    finally:
        for var in env:
            delenv(var)
    work.check_answers(index)
    return shape_of(index, "aux_budget_bytes" in options)


def observe_rebuild(work):
    index = gpu_index(work.texts, work.alphabet)
    shapes = [shape_of(index, False)]
    work.check_answers(index)
    for options in REBUILD_STEPS:
        index.rebuild_aux(**options)
        shapes.append(shape_of(index, False))
        work.check_answers(index)
    return shapes


@pytest.fixture(scope="module")
def workloads():
    return make_workloads()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_index_shape_is_the_recorded_one(name, workloads, golden, monkeypatch):
    for key, work in workloads.items():
        got = observe_case(name, work, monkeypatch.setenv, monkeypatch.delenv)
        assert got == golden[key][name], (key, name)
    if name == "seed12_budget_1000":  # an explicit k whose smallest table cannot fit is refused, with the existing message
        assert golden["dna"][name]["refused"] == _lib.GDX_ERR_INVALID_ARGUMENT and REFUSED in golden["dna"][name]["message"]
    if name == "defaults":
        assert golden["dna"][name]["default_shape"] and not golden["binary"][name]["default_shape"]


def test_rebuild_from_the_default_shape_to_tables_and_back(workloads, golden):
    for key, work in workloads.items():
        got = observe_rebuild(work)
        assert got == golden[key]["rebuild"], key
    first, tables, again = golden["dna"]["rebuild"]
    assert first == again and first["default_shape"] and not tables["default_shape"] and tables["jump_entry_bytes"] == 32
