"""The yardstick of the several-lights tests (tests/lights_model.py) pinned to
the oracle on the CPU: with one white light the model is the oracle's light
map, unfiltered and filtered, bit for bit; and the test lights are not
degenerate (leaves shared between lights, sums that depend on the order)."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt

import lights_model as lm

DEPTHS = (4, 6)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def proxy_small():
    return vrt.SceneData.proxy(0.25, 2)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("filt", [False, True])
def test_one_white_light_is_the_oracles_map(proxy_small, depth, filt):
    A = lm.issue_lights(vrt.to_radian)[0]
    osc = po.Scene(proxy_small, depth)
    want_hits = osc.lightmap(po.camera(*A.cam), 1.0, 1.0, *A.film, nthreads=8, filter=filt)
    wk, wcov, will = osc.lightmap_nodes()
    hits, (k, cov, ill) = lm.lightmap(po.Scene(proxy_small, depth), ("model", depth), [A], filter=filt)
    assert hits == want_hits == 1353
    assert np.array_equal(k, wk)
    assert np.array_equal(bits(cov), bits(wcov))
    assert np.array_equal(bits(ill), bits(will))
    assert bits(ill).any() and (cov.any() or not filt)


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_test_lights_are_not_degenerate(proxy_small, depth):
    A, B, C, Z = lm.issue_lights(vrt.to_radian)
    osc, key = po.Scene(proxy_small, depth), ("model", depth)
    hits = [lm.accumulate(osc, key, [l])[0] for l in (A, B, C, Z)]
    shared = (lm.shared_leaves(osc, key, [A, B]), lm.shared_leaves(osc, key, [A, B, C]))
    order = (lm.order_sensitive(osc, key, [A, B], [B, A]), lm.order_sensitive(osc, key, [A, B, C], [C, B, A]))
    print(f"depth {depth}: hits {hits}, shared leaves {shared}, order-sensitive nodes {order}")
    assert hits == [1353, 1021, 2766, 0]
    assert min(shared) >= 50
    assert min(order) >= 20
    assert np.isfinite(lm.lightmap(osc, key, [A, B, C])[1][2]).all()
    # a colour is one multiplication: B white and B coloured differ, and a
    # white B is the oracle's B
    white = lm.lightmap(osc, key, [B.white()], filter=False)[1][2]
    assert not np.array_equal(bits(white), bits(lm.lightmap(osc, key, [B], filter=False)[1][2]))
    o2 = po.Scene(proxy_small, depth)
    o2.lightmap(po.camera(*B.cam), 1.0, 1.0, *B.film, nthreads=8, filter=False)
    assert np.array_equal(bits(white), bits(o2.lightmap_nodes()[2]))
