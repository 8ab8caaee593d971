"""The two plain functions behind ``_lib.HostCall`` (the pinned host-block protocol of the one-wait calls: include/lvdgs.h, "Host blocks"):
the sequence counter's step and the verdict on a block's tag word.  No GPU and no pinned memory."""
import numpy as np
import pytest

from lvdgs import _lib


def test_the_counter_wraps_past_zero():
    assert _lib.next_seq(0) == 1 and _lib.next_seq(1) == 2
    assert _lib.next_seq(0x7FFFFFFE) == 0x7FFFFFFF and _lib.next_seq(0x7FFFFFFF) == 1
    for seq in (0, 1, 0x7FFFFFFD, 0x7FFFFFFE, 0x7FFFFFFF):
        assert 1 <= _lib.next_seq(seq) <= 0x7FFFFFFF      # never 0 (a cleared tag word), always an int32
    seq = 0x7FFFFFFC
    for want in (0x7FFFFFFD, 0x7FFFFFFE, 0x7FFFFFFF, 1, 2):
        seq = _lib.next_seq(seq)
        assert seq == want


def test_the_verdict_accepts_the_sequence_number_or_a_listed_status():
    words = np.array([5, 11, 12, 13], dtype=np.int32)
    assert _lib.host_block_verdict(words, "lvdgs_some_call", 0, seq=5) == 5
    assert _lib.host_block_verdict(words, "lvdgs_some_call", 2, seq=12) == 12      # the tag need not be word 0
    assert _lib.host_block_verdict(words, "lvdgs_some_call", 0, statuses=(4, 5)) == 5
    assert _lib.host_block_verdict(np.array([0x7FFFFFFF], dtype=np.int32), "lvdgs_some_call", 0, seq=0x7FFFFFFF) == 0x7FFFFFFF


@pytest.mark.parametrize("found, kw, expectation", [
    (0, dict(seq=5), "sequence number 5"),            # the cleared word: the call wrote nothing
    (4, dict(seq=5), "sequence number 5"),            # the call before
    (-7, dict(seq=1), "sequence number 1"),
    (0, dict(statuses=(1, 2)), "status 1 or 2"),
    (3, dict(statuses=(1, 2)), "status 1 or 2"),
    (5, dict(statuses=(1,)), "status 1"),
])
def test_the_verdict_refuses_anything_else(found, kw, expectation):
    words = np.array([found, 1, 2, 5], dtype=np.int32)      # (the expected values elsewhere in the block do not count)
    with pytest.raises(_lib.LvdgsError) as e:
        _lib.host_block_verdict(words, "lvdgs_some_call", 0, **kw)
    text = str(e.value)
    assert "lvdgs_some_call" in text and f"holds {found}," in text and expectation in text
