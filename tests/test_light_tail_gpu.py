"""The light pass's budget hand-off (ray_march<.., kBudget> -> k_light_tail)
as it happens by itself, counted by vrt_lightmap_stats, and light films that
are not square multiples of 64.  Bar: the light map bit-exact vs the oracle's
canonical-order sums.  The cases' conditions: cone_path_cases.py,
test_cone_paths_host.py."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt

import cone_path_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def proxy_small():
    return vrt.SceneData.proxy(0.25, 2)


def _build(tree, osc, light, nx, ny):
    """Both light maps; the hits and the product's map, equal to the oracle's."""
    hits = tree.lightmap(vrt.Camera(*light), vrt.Film(1, 1, nx, ny))
    assert hits == osc.lightmap(po.camera(*light), 1.0, 1.0, nx, ny, nthreads=8)
    got, want = tree.lightmap_nodes(), osc.lightmap_nodes()
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(cc.bits(got[1]), cc.bits(want[1]))
    assert np.array_equal(cc.bits(got[2]), cc.bits(want[2]))
    st = tree.lightmap_stats()
    assert st["samples"] == 64 * (nx // 8) * (ny // 8) * 4 and st["hits"] == hits
    return hits, got, st


# ---- G. the natural hand-off -----------------------------------------------------
@pytest.mark.parametrize("depth,n", [(5, 96), (4, 64)])
def test_light_budget_hand_off(proxy_small, depth, n):
    """No test flag: in the same waves some samples pass VRT_LIGHT_BUDGET
    triangle tests mid-walk and go to k_light_tail while others hit and
    record.  The kernel counts the records of the leaves it opens, the oracle
    those of every leaf on the ray, so the oracle's count of samples over the
    budget bounds the kernel's.  Measured on an MI355X: 32 of 36,864 samples
    deferred at depth 5 / 96 x 96 (the oracle: 188 over the budget), 200 of
    16,384 at depth 4 / 64 x 64 (365)."""
    tree, osc = vrt.VoxelOctree(proxy_small, depth), po.Scene(proxy_small, depth)
    assert tree.lightmap_stats() == {"samples": 0, "hits": 0, "deferred": 0}
    tests, _, _ = cc.light_tests(osc, cc.LIGHT, n, n)
    over = int((tests > cc.LIGHT_BUDGET).sum())
    hits, natural, st = _build(tree, osc, cc.LIGHT, n, n)
    print(f"depth {depth}, film {n}: {st}, oracle samples over the budget {over}")
    assert hits > 0
    assert 0 < st["deferred"] < st["samples"]
    assert st["deferred"] <= over
    # every sample to the tail: the same light map
    vrt.set_test_flags(vrt.TEST_LIGHT_TAIL)
    try:
        _, forced, st_all = _build(tree, osc, cc.LIGHT, n, n)
    finally:
        vrt.set_test_flags(0)
    assert st_all["deferred"] == st_all["samples"] == st["samples"]
    for a, b in zip(natural, forced):
        assert np.array_equal(cc.bits(a), cc.bits(b))


# ---- H. light-film shapes ---------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(104, 72), (100, 70)])
def test_light_film_not_square(proxy_small, nx, ny):
    """104 x 72: tasks of 13 x 9 pixels, the canonical key's tx * 8 + ty on a
    film that is not square.  100 x 70: no multiple of 8, the render area is
    96 x 64."""
    tree, osc = vrt.VoxelOctree(proxy_small, 5), po.Scene(proxy_small, 5)
    hits, _, st = _build(tree, osc, cc.LIGHT, nx, ny)
    assert hits > 0
    res = tree.min_voxel(6)
    fx, fy = cc.FRAME
    got = tree.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, fx, fy), res)
    want = osc.render_trace(po.camera(*cc.VIEW), 1.0, 1.0, fx, fy, res, samples=False)
    assert np.array_equal(cc.bits(got), cc.bits(want))


def test_light_film_all_miss(proxy_small):
    """The light camera turned away: no hit, so no sort and no sums; every
    illum is +0, the coverage is the filter's, and a frame on that map
    matches."""
    tree, osc = vrt.VoxelOctree(proxy_small, 5), po.Scene(proxy_small, 5)
    # after a lit map on the same scene, so that nothing of it may remain
    _build(tree, osc, cc.LIGHT, 64, 64)
    _build(tree, osc, cc.LIGHT, 64, 64)  # (both of the scene's two sets)
    for _ in range(2):
        hits, (_, cov, ill), st = _build(tree, osc, cc.LIGHT_AWAY, 64, 64)
        assert hits == 0 and st == {"samples": 16384, "hits": 0, "deferred": 0}
        assert np.all(cc.bits(ill) == 0) and cov[0] > 0
        res = tree.min_voxel(6)
        fx, fy = cc.FRAME
        got = tree.render_trace(vrt.Camera(*cc.VIEW), vrt.Film(1, 1, fx, fy), res)
        want = osc.render_trace(po.camera(*cc.VIEW), 1.0, 1.0, fx, fy, res, samples=False)
        assert np.array_equal(cc.bits(got), cc.bits(want))


def test_light_one_leaf_one_run():
    """One triangle at depth 1: the root is the only leaf and holds every
    hit, one sequential chain of sums whose length is no multiple of
    kLmBatch (8)."""
    sd = cc.one_triangle()
    tree, osc = vrt.VoxelOctree(sd, 1), po.Scene(sd, 1)
    assert tree.info.nodes == 1
    hits, (_, cov, ill), st = _build(tree, osc, cc.LIGHT, 64, 64)
    assert hits > 64 and hits % 8 != 0
    assert np.any(ill != 0) and cc.bits(cov)[0] == cc.bits(np.float32(1))[0]
    # (and the forced tail on the same single leaf)
    vrt.set_test_flags(vrt.TEST_LIGHT_TAIL)
    try:
        _build(tree, osc, cc.LIGHT, 64, 64)
    finally:
        vrt.set_test_flags(0)
