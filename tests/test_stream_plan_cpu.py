"""The stream plan of the resident queue (orb_geom.h: stream_plan), through rumi_hook_stream_plan: how many slot streams the queue drives for
the slots a caller asks for and the hardware queues of the process, and whether a slot's blur runs on the slot's own stream.

The rule, restated here from its description and not from the code:
    streams     = min(requested, max(2, hw_queues - reserve))
    blur inline = 2 * streams + reserve > hw_queues      (slot + blur streams + reserve would not fit the queues)
with reserve = 0 or 1 queues left to the caller's stream (a measured choice the hook reports)."""
import ctypes as C
import os

import pytest

from rumi_slam_amd import capi

HW = range(1, 33)
SLOTS = range(2, 9)


def plan(requested, hw):
    H = capi.hooks()
    s, b, r = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert H.rumi_hook_stream_plan(requested, hw, C.byref(s), C.byref(b), C.byref(r)) == 0
    return s.value, b.value, r.value


def test_reserve_is_zero_or_one():
    assert plan(4, 4)[2] in (0, 1)


@pytest.mark.parametrize("hw", HW)
def test_plan_follows_the_rule(hw):
    for req in SLOTS:
        streams, inline, reserve = plan(req, hw)
        assert 1 <= streams <= req
        if hw >= 2 + reserve:
            assert streams + reserve <= hw
        assert streams == min(req, max(2, hw - reserve))
        assert inline == (1 if 2 * streams + reserve > hw else 0)


def test_blur_streams_return_when_the_queues_have_room():
    _, _, reserve = plan(4, 4)
    assert plan(4, 4)[1] == 1                            # four queues: nine streams never fitted
    assert plan(4, 8 + reserve) == (4, 0, reserve)       # room for four slot streams, four blur streams and the reserve
    assert plan(4, 8 + reserve - 1)[1] == 1


def test_unset_and_unparsable_mean_four():
    H = capi.hooks()
    assert H.rumi_hook_parse_hw_queues(None) == 4
    for bad in (b"", b"four", b"4x", b"0", b"-3", b" ", b"1e1", b"99999999999999999999"):
        assert H.rumi_hook_parse_hw_queues(bad) == 4, bad
    for v in (1, 2, 4, 8, 24, 32):
        assert H.rumi_hook_parse_hw_queues(str(v).encode()) == v


def test_environment_answer_is_the_parsed_one():
    """hw_queues <= 0 asks for the plan of this process's own GPU_MAX_HW_QUEUES (read once by the library, never set by it): the answer for an
    unset variable is the one for four queues, for an unparsable one too."""
    H = capi.hooks()
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    v = before.encode() if before is not None else None
    hw = H.rumi_hook_parse_hw_queues(v)
    if before is None:
        assert hw == 4
    for req in SLOTS:
        assert plan(req, 0) == plan(req, hw)
    assert os.environ.get("GPU_MAX_HW_QUEUES") == before
