"""GPU: a Flow2Batch keeps its context alive (ba.Context._retain / _release), as BatchBA does: vdo_flow2_batch_destroy waits on the context's
stream.  Python gives no order among the finalisers of one garbage-collected cycle - the frames a pytest.raises keeps, for instance - so a
context closed or finalised BEFORE its batches must postpone its own destroy until they have let go."""
import pytest

pytestmark = pytest.mark.gpu


def test_a_context_closed_first_waits_for_its_flow2_batches():
    from vdo_slam_amd import synth
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.flow2 import Flow2Batch
    ctx = Context(0)
    b = Flow2Batch(ctx, [synth.make_flow2_problem(200, seed=3)])
    r = Flow2Batch.reserve(ctx, [16, 16])
    assert ctx._users == 2
    ctx.close()
    assert ctx._h and ctx._close_pending                    # postponed: two users
    b.run()
    assert b.fetch()[0]["iterations"] >= 1                  # and the batch still has its stream
    b.close()
    assert ctx._h and ctx._users == 1
    b.close()                                               # a second close releases nothing
    assert ctx._users == 1
    r.close()
    assert not ctx._h and ctx._users == 0                   # the last user's close destroyed the context


def test_a_refused_create_retains_nothing():
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.flow2 import Flow2Batch
    ctx = Context(0)
    with pytest.raises(K.VdoError):
        Flow2Batch.reserve(ctx, [10, -1])
    assert ctx._users == 0
    ctx.close()
    assert not ctx._h
