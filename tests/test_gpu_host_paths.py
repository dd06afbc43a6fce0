"""Every result path of the host-pointer pipeline (genedex_amd/csrc/host_api.hip) on one small batch: exact intervals, counts,
the plain locate (u64 offsets), the fused step with device-written results and the fused step with the found-bitmap wire, each
from ASCII, caller-packed, uniform and packed + uniform queries, with chunks small enough that every one of the four slots is
used more than twice.  The batch holds reads with no, one and several hits, empty reads, a run of reads with an N (those
chunks go as ASCII, the others as 2-bit codes), one read longer than a chunk's byte limit, and a cluster of one- and two-symbol
reads whose chunk has more hits than its device buffers were sized for (the second half of the step runs again).  Answers are
the oracle's.  The index, the batches and the checks live in host_paths_child.py, which is also the program the per-process
switches are tested with."""
import os
import subprocess
import sys

import pytest

import host_paths_child as hp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (97 reads a chunk: 4 * 97 for the fused step, ten chunks or more of it and about forty of the count path; the second: the
# byte rule cuts -- 1500 bytes of ASCII, 6000 symbols of 2-bit codes -- and the long read is a chunk of its own)
CHUNKINGS = [(97, 0), (512, 1500)]


@pytest.fixture(scope="module")
def case():
    return hp.build_case()


@pytest.fixture
def chunking(case, request):
    case.lib.gdx_debug_set_host_chunking(*request.param)
    try:
        yield request.param
    finally:
        case.lib.gdx_debug_set_host_chunking(0, 0)


@pytest.mark.parametrize("chunking", CHUNKINGS, indirect=True, ids=["97-reads", "1500-bytes"])
@pytest.mark.parametrize("form", ["ascii", "packed", "uniform", "packed-uniform"])
def test_every_call_gives_the_oracles_result(case, chunking, form):
    hp.check_form(case, case.forms[form])


@pytest.mark.parametrize("chunking", CHUNKINGS, indirect=True, ids=["97-reads", "1500-bytes"])
def test_one_bad_read_in_the_middle_chunk(case, chunking):
    hp.check_statuses(case)


@pytest.mark.parametrize("chunking", CHUNKINGS[:1], indirect=True, ids=["97-reads"])
@pytest.mark.parametrize("form", ["ascii", "uniform"])
def test_without_host_packing(case, chunking, form, monkeypatch):
    """GDX_HOST_PACK=0 (read per call): ASCII chunks cross the link as they are"""
    monkeypatch.setenv("GDX_HOST_PACK", "0")
    hp.check_form(case, case.forms[form])


@pytest.mark.parametrize("chunking", CHUNKINGS[:1], indirect=True, ids=["97-reads"])
@pytest.mark.parametrize("form", ["ascii", "packed-uniform"])
def test_chunk_hit_limit_sends_the_wide_calls_through_the_retry(case, chunking, form, monkeypatch):
    """GDX_TEST_CHUNK_HIT_LIMIT=50 (read per call) stands in for 2^32 - 1 hits in a chunk: the fused step of a wide locate gives
    up at the first chunk, its three threads stop, and the call runs again on the plain path; the narrow call has no such
    limit and the sizing call never takes the step"""
    monkeypatch.setenv("GDX_TEST_CHUNK_HIT_LIMIT", "50")
    hp.check_form(case, case.forms[form], flagged=False)


@pytest.mark.parametrize("env", [{"GDX_HOST_RESULTS": "wire"}, {"GDX_HOST_RESULTS": "dma"},
                                 {"GDX_HOST_RESULTS": "dma", "GDX_HOST_WIDE_HITS": "1"}],
                         ids=["wire", "dma", "dma-wide-hits"])
def test_per_process_switches_in_a_fresh_process(env):
    """wire: the found-bitmap wire for the narrow and the wide calls.  dma: the narrow call with device-written offsets and
    hits, the wide calls on the plain path with 8-byte hits widened by the drainer -- or (GDX_HOST_WIDE_HITS=1) 16-byte hits
    from the device"""
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("GDX_")}
    child_env.update(env)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_paths_child.py")], cwd=ROOT, env=child_env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("PASS"), res.stdout[-2000:] + res.stderr[-3000:]
