"""GPU tests of the chain order (expand_v2<2, true>,
chain_criterion, chain_order2 / chain_order4 in vrt_kernels.hip): the walk's
own code on the input families of tests/chain_order_cases.py
(vrt_device_selftest_chain), small frames of the proxy scene through the
production launch, and adversarial rays through vrt_ray_march_batch -- all
against the oracle."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt
import chain_order_cases as cc

pytestmark = pytest.mark.gpu

F = np.float32
LEAF_BIT = np.uint32(0x80000000)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_build_flag():
    assert vrt.build_flag("VRT_CHAIN_ORDER") == 1


# ------------------------------------------------------------- (a) the code
SIZES = {"random": 8000, "near_axis": 6000, "diagonal": 2000, "features": 2000, "far": 2000}


@pytest.fixture(scope="module")
def selftest():
    """Every family once through vrt_device_selftest_chain: name -> (host
    restatement, device words)."""
    wmin = cc.scene_spacing()
    fams = {k: cc.FAMILIES[k](10 + i, n) for i, (k, n) in enumerate(SIZES.items())}
    assert sum(SIZES.values()) <= 20_000
    rows = np.concatenate([cc.device_cases(f, wmin) for f in fams.values()])
    out = vrt.device_selftest_chain(rows)
    res, at = {}, 0
    for k, f in fams.items():
        n = f[0].shape[0]
        res[k] = (cc.evaluate(f, wmin), out[at:at + n])
        at += n
    return res


@pytest.mark.parametrize("family", list(SIZES))
def test_selftest_equals_the_restatement_and_the_sort(selftest, family):
    ev, out = selftest[family]
    cnt = ev["cnt"]
    assert np.all(out[:, 4] & 8)  # every ray meets the finite-slab walk's preconditions
    assert np.array_equal(out[:, 0], ev["hm"])
    assert np.array_equal(out[:, 1] >> 24, cnt.astype(np.uint32))
    crit, chain = (out[:, 4] & 1) != 0, (out[:, 4] & 2) != 0
    assert np.array_equal(crit, ev["crit"])
    assert np.array_equal(chain, ev["chain"])
    assert np.array_equal((out[:, 4] & 4) != 0, ev["chain"])  # the general form agrees on every count
    both = crit & chain
    # wherever both flags are set the chain order is the sort's order
    assert np.array_equal(out[both, 2], out[both, 1])
    assert np.array_equal(out[chain, 3], out[chain, 2])
    # ... and the restatement's
    want = cc.pack(ev["order"], cnt) | (cnt.astype(np.uint32) << 24)
    assert np.array_equal(out[chain, 2], want[chain])
    # the walk's own expansion (wave votes, fallback) always gives the sort's order
    assert np.array_equal(out[:, 5], out[:, 1])
    multi = cnt >= 2
    print(f"{family}: {int(multi.sum())} cases with >= 2 hit children, {int((multi & both).sum())} by the chain order")
    if family == "random":
        assert (multi & both).sum() >= 0.90 * multi.sum()
    if family == "near_axis":
        assert (multi & ~crit).sum() >= 0.25 * multi.sum()
    if family == "far":
        assert not np.any(crit)


# --------------------------------------------------------------- (b) frames
# (proxy detail, depth, record bytes): at depths 5 and 6 the full proxy has
# >= 8 records per leaf (64-B records: the production launch is the one-wave
# grid, no chain order); the coarser proxies keep 48-B records, so their
# production launch is k_render_p<true> with the chain order
SCENES = [(1.0, 5, 64), (1.0, 6, 64), (0.02, 6, 48), (0.1, 7, 48)]


@pytest.fixture(scope="module", params=SCENES, ids=lambda p: "detail%g-depth%d" % p[:2])
def proxy(request):
    detail, d, rec = request.param
    sd = vrt.SceneData.proxy(detail, 1)
    return rec, vrt.VoxelOctree(sd, d), po.Scene(sd, d)


def _cameras(tree):
    """Poses 0 and (sheared, as test_leaf_cull_gpu.py) 5 of the sweep; an
    axis-aligned camera at the scene's height looking along -z, whose central
    row and column make near-axis rays; a camera 150 extents outside."""
    mn, mx = tree.root_box
    cen = (mn.astype(np.float64) + mx) * .5
    ext = float(np.max(mx - mn))
    out = []
    for pose, shear in ((0, None), (5, {1: 0.75, 5: -1.0 / 64, 9: 0.0})):
        fov, eye, spot, up = vrt.sweep_pose(mn, mx, pose, 16)
        cam, ocam = vrt.Camera(fov, eye, spot, up), po.camera(fov, eye, spot, up)
        for k, v in (shear or {}).items():
            cam.c.C[k] = v
            ocam[k] = v
        out.append(("pose%d" % pose, cam, ocam))
    axis = (vrt.to_radian(60), cen + [0, 0, 0.9 * ext], cen, (0, 1, 0))
    far = (vrt.to_radian(0.6), cen + ext * np.array([90.0, 60.0, 105.0]), cen, (0, 1, 0))
    for name, (fov, eye, spot, up) in (("axis", axis), ("far", far)):
        e, s, u = F(eye), F(spot), F(up)
        out.append((name, vrt.Camera(fov, e, s, u), po.camera(fov, e, s, u)))
    return out


@pytest.mark.parametrize("size", [64, 128])
def test_frames_equal_the_oracle(proxy, size):
    """Every sample's hit, triangle and voxel ids and RGB bits (vrt_render's
    per-sample outputs) and the film of the production launch
    (vrt_render_tiles_device: k_render_p<true> with the chain order) equal the
    oracle's."""
    import torch
    rec, tree, osc = proxy
    assert tree.ref_record_bytes == rec and np.all(tree.chain_spacing > 0)
    film = vrt.Film(1, 1, size, size)
    dev = torch.device("cuda:0")
    for name, cam, ocam in _cameras(tree):
        wrgb, wso = osc.render(ocam, 1.0, 1.0, size, size, film_index=1, nthreads=16, samples=True)
        rgb, so = tree.render(cam, film, samples=True)
        for key in ("hit", "tri", "voxel"):
            assert np.array_equal(so[key], wso[key]), (name, key)
        assert np.array_equal(bits(so["rgb"]), bits(wso["rgb"])), name
        assert np.array_equal(bits(rgb), bits(wrgb)), name
        img = torch.zeros((size, size, 3), dtype=torch.float32, device=dev)
        tree.render_tiles_device(cam, film, 0, 1, 1, img.data_ptr(), None)
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(wrgb)), (name, "film")
        if name != "far":
            assert wso["hit"].mean() > 0.2, name


# ----------------------------------------------------- (c) adversarial rays
def _soup():
    """A few hundred small triangles scattered in a non-cubic box: an octree
    of depth 4 with internal nodes at every level."""
    rng = np.random.default_rng(7)
    lo, hi = np.array([-0.8, 0.1, -1.9]), np.array([1.3, 1.2, 0.4])
    c = lo + rng.random((400, 1, 3)) * (hi - lo)
    pos = (c + (rng.random((400, 3, 3)) - .5) * 0.12).reshape(400, 9).astype(F)
    return vrt.SceneData(pos, np.tile(F([0, 0, -1]), (len(pos), 3)))


@pytest.fixture(scope="module")
def soup():
    sd = _soup()
    return vrt.VoxelOctree(sd, 4), po.Scene(sd, 4)


@pytest.mark.parametrize("family", list(SIZES))
def test_ray_march_batch_equals_the_oracle(soup, family):
    """1000 rays of each family aimed at the soup's internal nodes, through
    vrt_ray_march_batch (k_ray_march<false>: the chain order where the wave's
    rays pass the criterion): hit, triangle, voxel and the hit point and
    normal bits equal the oracle's."""
    tree, osc = soup
    box, a, _ = tree.nodes()
    inner = (a & LEAF_BIT) == 0
    nodes = (box[inner, :3], box[inner, 3:])
    mn, mx = tree.root_box
    wmin = tree.chain_spacing
    assert np.all(wmin > 0)
    origin = mn + F([0.37, 0.55, 0.61]) * (mx - mn)
    fam = cc.FAMILIES[family](20, 1000, nodes=nodes, origin=origin, root=(mn, mx))
    bmin, bmax, o, d = fam
    rays = np.ascontiguousarray(np.concatenate(
        [o, d, np.zeros((len(o), 1), F), np.full((len(o), 1), vrt.FLT_MAX, F)], 1), F)
    assert np.all(rays[:, 3:6] != 0)
    crit = cc.criterion(np.tile(mn, (len(o), 1)), np.tile(mx, (len(o), 1)), o, d, wmin)
    print(f"{family}: {int(crit.sum())} of {len(o)} rays pass the criterion")
    want = osc.ray_march(rays)
    got = tree.ray_march(rays)
    for key in ("hit", "tri", "voxel"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(bits(got["hit_p"]), bits(want["hit_p"]))
    assert np.array_equal(bits(got["normal"]), bits(want["normal"]))
    if family in ("random", "features"):
        assert want["hit"].sum() > 50
