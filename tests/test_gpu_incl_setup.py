"""The inclusion pass of the split fresh read (csrc/am_group_split.h k_grp_incl) sets up a wave batch's
32 reads at once: lane j computes read j's thresholds, lag bases and window limits (am_iw_read_setup,
csrc/am_inclwin.h) into its LDS slot, the reads' loops take them from there, and the batch's LastOpCt
rows are u32 maxima above the slot's K, widened as the columns are stored.  The logs of
tests/incl_setup_cases.py put one or two batches where a slot can go wrong: neighbouring keys with
other time bases and other lag bases on every DC, eligible slots between hand-offs, a routed key and
an error status, clocks below K, without a DC, above and below every op, bounds carried across
segments, and escaped ops whose maxima need the merge in 64 bits.  Every batch is read three ways
(test_gpu_inclwindow.three_ways): the lag view, the same device log with lag_ct nulled (the packed
instantiation; every column and the pairs bit-equal) and the C oracle.  tests/test_incl_setup_cpu.py
asserts on the host that the same logs and clocks meet each of these."""
import pytest

from antidote_amd import abi
from tests.incl_setup_cases import case
from tests.test_gpu_inclwindow import three_ways

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def run_case(mat, name, t, n_dc, routed=0, lag_only=None, pk_esc=None):
    keys, log, clocks = case(name, t, n_dc)
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        stats = st.view_stats()
        assert stats["routed_keys"] == routed, stats
        if lag_only is not None:
            assert stats["lag_only_esc_ops"] == lag_only and stats["pk_esc_ops"] == pk_esc, stats
        dlog = st.device_log()
        assert dlog.lag_ct and not dlog.zone_vc
        for clock, pres in clocks:
            three_ways(mat, dlog, log, keys, t, n_dc, clock, pres)
    finally:
        st.close()


# n_dc 5: no template width, the runtime-width instantiation of D = 8 (pad DCs)
@pytest.mark.parametrize("t,n_dc", [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3), (abi.AM_MVREG, 3),
                                    (abi.AM_AWSET, 5), (abi.AM_MVREG, 5)])
def test_gpu_incl_setup_mixed_keys(mat, t, n_dc):
    run_case(mat, "mixed", t, n_dc, lag_only=0, pk_esc=0)


def test_gpu_incl_setup_clock_edges(mat):
    run_case(mat, "edges", abi.AM_AWSET, 8, lag_only=0, pk_esc=0)


@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_gpu_incl_setup_sparse_batch(mat, t):
    run_case(mat, "sparse", t, 8, routed=2)


def test_gpu_incl_setup_segments(mat):
    run_case(mat, "segments", abi.AM_AWSET, 8, lag_only=0, pk_esc=0)


@pytest.mark.parametrize("t,n_dc", [(abi.AM_AWSET, 8), (abi.AM_MVREG, 3)])
def test_gpu_incl_setup_escapes(mat, t, n_dc):
    run_case(mat, "escapes", t, n_dc, lag_only=1, pk_esc=3)
