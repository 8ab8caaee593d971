"""``_lib.HostCall`` on the GPU: the owner of the pinned host block, the scratch and the one wait of the calls that report through such a
block (include/lvdgs.h, "Host blocks").  A call that writes nothing is refused whatever the call before left in the block; the
resources are kept and grown; ``lvdgs_pnp_ransac`` writes every word of its block.  The smallest shapes: every test is a few launches."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# 8 matches on a 16 x 16 raster of constant depth 2.0, 8 hypotheses; the new frame sees every match where the keyframe does
PIXELS = np.array([(2, 3), (5, 4), (9, 2), (12, 6), (3, 10), (7, 12), (11, 11), (13, 14)], dtype=np.int32)
K = (16.0, 16.0, 8.0, 8.0)


def nothing(args, stream):
    """A stand-in for a library function: reports success, launches nothing, writes nothing."""
    return 0


def pnp_call():
    from lvdgs import _lib, init_pose
    init_pose.pnp_ransac(torch.full((16, 16), 2.0, device=DEV), PIXELS, PIXELS.astype(np.float32), K, hypotheses=8)
    assert init_pose.last_call.status in (_lib.PNP_OK, _lib.PNP_FAILED)
    return init_pose._pnp


def summary_call():
    from lvdgs import frame_stats
    pkg = dict(depth=torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV), opacity=None, n_touched=torch.zeros(0, dtype=torch.int32, device=DEV))
    fs = frame_stats.frame_summary(pkg, [])
    assert fs.visible == 0 and fs.covis == {}
    return frame_stats._summary


def test_a_stale_status_block_is_refused():
    """The block holds a valid status of the call before; a call that writes nothing must not be taken for one that ended in it."""
    from lvdgs import _lib
    call = pnp_call()
    block = call.blocks[DEV.index]
    assert int(block.numpy().view(np.int32)[0]) in (_lib.PNP_OK, _lib.PNP_FAILED)
    with pytest.raises(_lib.LvdgsError, match="lvdgs_pnp_ransac left no state"):
        call.run(DEV, _lib.PnpArgs(host_state=block.data_ptr()), nothing)


def test_a_stale_sequence_block_is_refused():
    from lvdgs import _lib
    call = summary_call()
    block = call.blocks[DEV.index]
    seq = call.seq[DEV.index]
    assert int(block.numpy().view(np.int32)[_lib.FRAME_SUMMARY_SEQ]) == seq >= 1
    with pytest.raises(_lib.LvdgsError, match="lvdgs_frame_summary left no state"):
        call.run(DEV, _lib.FrameSummaryArgs(host_state=block.data_ptr()), nothing)
    assert call.seq[DEV.index] == _lib.next_seq(seq)      # the refused call had a number of its own


def test_resources_are_kept_and_grown():
    from lvdgs import _lib
    call = _lib.HostCall("lvdgs_pnp_ransac", statuses=(_lib.PNP_OK, _lib.PNP_FAILED))
    block, scratch = call.resources(DEV, 128, 1000)
    assert block.is_pinned() and block.numel() >= 128 and scratch.device == DEV and scratch.numel() >= 1000
    block2, scratch2 = call.resources(DEV, 128, 5000)      # more scratch than the call before
    assert scratch2.numel() >= 5000 and block2.data_ptr() == block.data_ptr()
    block3, scratch3 = call.resources(DEV, 64, 300)        # less of both: what is there is large enough
    assert block3.data_ptr() == block.data_ptr() and scratch3.data_ptr() == scratch2.data_ptr()
    assert call.resources(DEV, 4096)[0].numel() >= 4096 and call.resources(DEV, 64)[1] is None
    roomy = _lib.HostCall("lvdgs_map_edit_plan", headroom=True, zeroed=True)
    block, scratch = roomy.resources(DEV, 1000, 2000)
    assert block.numel() >= 1500 and scratch.numel() >= 3000 and not bool(scratch.any())


def test_entry_points_do_not_share_a_block():
    pnp, summary = pnp_call(), summary_call()
    a, b = pnp.blocks[DEV.index], summary.blocks[DEV.index]
    assert a.data_ptr() != b.data_ptr()
    assert pnp_call().blocks[DEV.index].data_ptr() == a.data_ptr() and summary_call().blocks[DEV.index].data_ptr() == b.data_ptr()


def test_pnp_writes_every_word_of_its_block():
    """lvdgs_pnp_ransac on a block prefilled with -7 (as tests/test_gpu_recip_nn.py and test_gpu_matcher_io.py do for their calls): no
    state word and no pose double keeps the fill."""
    from lvdgs import _lib
    L = _lib.lib()
    depth = torch.full((16, 16), 2.0, device=DEV)
    m1, m2 = torch.from_numpy(PIXELS).to(DEV), torch.from_numpy(PIXELS.astype(np.float32)).to(DEV)
    mask = torch.full((8,), 7, dtype=torch.uint8, device=DEV)
    state = torch.full((_lib.PNP_HOST_BYTES // 4,), -7, dtype=torch.int32).pin_memory()
    scratch = torch.zeros(max(L.lvdgs_pnp_scratch_bytes(8, 8), 256), dtype=torch.uint8, device=DEV)
    a = _lib.PnpArgs(width=16, height=16, num_matches=8, hypotheses=8, min_inliers=6, seed=0, fx=K[0], fy=K[1], cx=K[2], cy=K[3],
                     reproj_error=5.0, depth=depth.data_ptr(), matches_im1=m1.data_ptr(), matches_im2=m2.data_ptr(),
                     inlier_mask=mask.data_ptr(), host_state=state.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    assert L.lvdgs_pnp_ransac(C.byref(a), _lib.raw_stream(DEV)) == _lib.OK, L.lvdgs_last_error()
    torch.cuda.synchronize(DEV)
    w = state.numpy()
    assert int(w[0]) in (_lib.PNP_OK, _lib.PNP_FAILED) and not (w[:_lib.PNP_STATE_WORDS] == -7).any(), w[:_lib.PNP_STATE_WORDS]
    pose = w[_lib.PNP_STATE_WORDS:].view(np.int64)
    fill = np.array([-7, -7], dtype=np.int32).view(np.int64)[0]
    assert pose.size == 12 and not (pose == fill).any()
