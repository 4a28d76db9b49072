"""The write path end to end on the device: two transactions update one PN key and prepare in one
batch (am_cert), the loser aborts, the winner commits and its effect goes through
am_vnode_commit_host; a read at the commit time sees the winner's value only, and the read servers'
check on the key holds a read back before the finish and lets it through after."""
import pytest

from antidote_amd import abi
from antidote_amd.oplog import Read
from tests.certsim import OK, WRITE_CONFLICT

pytestmark = pytest.mark.gpu

KEY, PN = 2, abi.AM_PN


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def test_gpu_cert_prepare_commit_read(mat):
    vn, c = mat.vnode(1, 4), mat.certifier(8, 8)
    try:
        updates = {11: 5, 12: 7}  # txid -> its increment of the key
        st = c.prepare([(11, 100, 110, True, [KEY]), (12, 100, 111, True, [KEY])])
        assert st == [OK, WRITE_CONFLICT]
        assert c.key_info(KEY) == (0, [(11, 110)]) and c.min_prepared() == 110
        assert c.read_ready([(KEY, 200), (KEY, 109), (KEY + 1, 200)], 300) == [10, 0, 0]
        # the loser aborts (it holds nothing here), the winner commits
        assert c.finish([(12, 0, False, [KEY])]) == [OK]
        assert c.key_info(KEY) == (0, [(11, 110)])
        assert c.read_ready([(KEY, 200)], 300) == [10]
        assert c.finish([(11, 120, True, [KEY])]) == [OK]
        vn.commit([(0, 120, {0: 100}, None, [(KEY, PN, updates[11])])])
        assert c.read_ready([(KEY, 200), (KEY, 400)], 300) == [0, 1]
        assert c.key_info(KEY) == (120, []) and c.min_prepared() is None
        r = vn.read([Read(KEY, PN, {0: 120})]).result(0)
        assert r[:2] == ("ok", updates[11])
        # the commit time now certifies against older snapshots
        assert c.prepare([(13, 119, 130, True, [KEY]), (14, 120, 131, True, [KEY])]) == [WRITE_CONFLICT, OK]
    finally:
        c.close()
        vn.close()
