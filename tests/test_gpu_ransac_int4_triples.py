"""ransac_run_dev above 2^21 source points, where a batch's index triples travel as int4 (i0, i1, i2, valid) and not as one
packed 64-bit word each (csrc/tdv_internal.hpp: triple_pack, kTriplePackMaxN).  One cloud of 2^21 + 1 points, a target that is
a rigid transform of it, supplied correspondences of which about 30 % are true; 20,000 iterations make a first batch and a
bounded second one.  The default call (bail-out and leaf bound), the traced call (every count on the host) and the exact-scoring
call return the same result to the bit, the default call left tests out, and the traced call's first counts are the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = 2 ** 21 + 1
ITERS = 20000
VOXEL = 0.01


def _result(r):
    return (r.transformation.tobytes(), r.inliers, np.float32(r.fitness).tobytes(), np.float32(r.rmse).tobytes(),
            r.best_iteration, r.iterations_run)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(2021)
    src = (rng.random((NS, 3)) - 0.5).astype(np.float32)
    ang = 0.7; ax = np.array([0.3, -0.5, 0.8]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    tgt = (src.astype(np.float64) @ R.T + np.array([0.05, -0.02, 0.1])).astype(np.float32)
    corr = np.where(rng.random(NS) < 0.3, np.arange(NS), rng.integers(0, NS, NS)).astype(np.int32)
    return src, tgt, corr


def test_int4_triples_default_traced_and_exact_agree(ctx, orc, scene):
    src, tgt, corr = scene
    got = ctx.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=ITERS, confidence=2.0)
    scored = ctx.last_ransac_scored()
    traced = ctx.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=ITERS, confidence=2.0, trace=True)
    try:
        ctx.set_ransac_score("exact")
        exact = ctx.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=ITERS, confidence=2.0)
    finally:
        ctx.set_ransac_score("fast")
    print("ns %d: best %d @ %d, run %d, fitness %r, scored %.3f" % (NS, got.inliers, got.best_iteration, got.iterations_run, got.fitness, scored))
    assert got.best_iteration >= 0 and got.iterations_run == ITERS
    assert _result(got) == _result(traced)
    assert _result(got) == _result(exact)
    assert scored < 1.0                      # the bail-out ran: the agreement above is not that of three full scorings
    ref = orc.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=32, confidence=2.0, trace=True)
    assert np.array_equal(traced.trace_inliers[:32], ref["inliers"])      # the index stream is sequential: the same first 32 triples
