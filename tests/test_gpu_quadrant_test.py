"""The blend kernels' two-step quadrant reach test (csrc/common.hpp: quad_prepare + reaches_rect_prepared) keeps exactly the
survivors reaches_rect() kept: on a scene built to stress it (tests/quadrant_scene.py) every image, count and gradient is, bit
for bit, what the library computed before the change (tests/golden/quadrant_test.npz, recorded with
tests/golden/make_quadrant_test_golden.py from the parent commit's build)."""
import numpy as np
import pytest

import quadrant_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    return quadrant_scene.collect()


@pytest.fixture(scope="module")
def golden():
    with np.load(quadrant_scene.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_scene_is_the_one_the_fixture_was_recorded_on_and_stages_several_rounds(results, golden):
    lengths = results["calls/list_lengths"]
    np.testing.assert_array_equal(lengths, golden["calls/list_lengths"])
    assert lengths.size == 24 and lengths[0] > 256 and lengths[3] > 64
    assert (results["calls/final_T"] > 1e-4).mean() > 0.9   # the lists are walked to their ends


def _names(golden, prefix):
    return sorted(k[len("meta:"):] for k in golden if k.startswith("meta:" + prefix))


def _compare(results, golden, prefix):
    names = _names(golden, prefix)
    assert names and set(names) == {k for k in results if k.startswith(prefix)}
    differing = []
    for k in names:
        v = np.ascontiguousarray(results[k])
        assert str(golden["meta:" + k]) == f"{v.dtype.str} {v.shape}", k
        if k in golden:
            same = np.array_equal(v.view(np.uint8), np.ascontiguousarray(golden[k]).view(np.uint8))
        else:
            same = np.array_equal(quadrant_scene.digest(v), golden["sha256:" + k])
        if not same:
            differing.append(k)
    assert not differing, f"differ from the parent build's bits: {differing}"


@pytest.mark.parametrize("prefix", ["calls/", "fused/mono/full/", "fused/mono/pose_only/", "fused/rgbd/full/", "fused/rgbd/pose_only/"])
def test_every_output_equals_the_parent_builds_bit_for_bit(results, golden, prefix):
    """calls/: lvdgs_forward + lvdgs_backward (colour, depth, opacity, n_contrib, n_touched; the full and the pose-only backward, with
    and without a depth gradient); fused/: lvdgs_forward_backward_fused_loss, both blend passes in one launch."""
    _compare(results, golden, prefix)
