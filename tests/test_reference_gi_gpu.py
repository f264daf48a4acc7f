"""The HIP paths against the reference's own recorded outputs
(tests/golden/ref_gi_*.npz: camera.cc and voxel_octree.cc compiled unmodified
and run by tests/golden/make_golden.py through oracle/ref_gi_glue.cc), with no
oracle in between: the builds' leaves, vrt_ray_march_batch[_ex], the primary
render's per-sample ids and colours, the node records of vrt_lightmap_build
and vrt_lightmap_build_lights, vrt_cone_trace_batch, vrt_trace_batch, the
trace() frame of the one-call entry, vrt_probe_gather and vrt_probe_eval.

Bar: identity.  Ids, hit flags and leaf codes are equal; every float is equal
in its bits (NaN matching NaN); nothing is excluded and nothing skips."""
import numpy as np
import pytest

import voxelraytrace20190722_amd as vrt
from conftest import golden

import ref_gi_record as rec
import reference_gi_cases as rc

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def sd():
    return rec.scene()


@pytest.fixture(scope="module")
def zm(sd):
    z = golden("ref_gi_march.npz")
    assert str(z["scene_sha"]) == str(rec.scene_sha(sd))
    return z


@pytest.fixture(scope="module")
def zl(sd):
    z = golden("ref_gi_light.npz")
    assert str(z["scene_sha"]) == str(rec.scene_sha(sd))
    return z


@pytest.fixture(scope="module")
def zp(sd):
    z = golden("ref_gi_probes.npz")
    assert str(z["scene_sha"]) == str(rec.scene_sha(sd))
    return z


def _film(z):
    f = z["film"]
    return vrt.Film(float(f[0]), float(f[1]), int(f[2]), int(f[3]))


def _light_film(z):
    n = int(z["light_n"])
    return vrt.Film(1, 1, n, n)


@pytest.fixture(scope="module")
def tree(sd, zm):
    return vrt.VoxelOctree(sd, int(zm["depth"]))


@pytest.fixture(scope="module")
def lit(sd, zl):
    """The scene under the white light map (state: built once, never relit)."""
    t = vrt.VoxelOctree(sd, int(zl["depth"]))
    hits = t.lightmap(vrt.Camera(*rec.cam_of(zl["light0_cam"])), _light_film(zl))
    assert hits == int(zl["white_hits"])
    return t


def _same_march(g, z, pre):
    assert np.array_equal(g["hit"], z[pre + "hit"]), (pre, "hit", int((g["hit"] != z[pre + "hit"]).sum()))
    for k in ("tri", "voxel"):
        assert np.array_equal(g[k], z[pre + k]), (pre, k, int((g[k] != z[pre + k]).sum()))
    for k in ("hit_p", "normal"):
        assert rc.same_f32(g[k], z[pre + k]), (pre, k, rc.diff_count(g[k], z[pre + k]))


def _keys(t):
    import probe_cases as pc
    box, a, _ = t.nodes()
    keys = pc.node_keys(a)
    return np.sort(keys), box[0]


# ---- the builds -------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["host_build", "device_build"])
def test_tree_leaves(sd, zm, zp, on_device):
    t = vrt.VoxelOctree(sd, int(zm["depth"]), build_on_device=on_device)
    for a, k in zip(t.leaves(), ("leaf_voxel", "leaf_count", "leaf_list")):
        assert np.array_equal(a, zm[k]), k
    keys, root = _keys(t)
    assert np.array_equal(keys, zm["node_key"]) and rc.same_f32(root, zm["root_box"])
    # the probe scene: probes behind the triangles in one tree
    p = vrt.VoxelOctree(sd, int(zp["probe_depth"]), build_on_device=on_device, probes=zp["scene_probes"])
    tl, pl = rec.split_leaves(zp["leaf_voxel"], zp["leaf_count"], zp["leaf_list"], sd.ntri)
    for got, want, what in ((p.leaves(), tl, "triangles"), (p.probe_leaves(), pl, "probes")):
        for a, b in zip(got, want):
            assert np.array_equal(a, b), what
    keys, root = _keys(p)
    assert np.array_equal(keys, zp["node_key"]) and rc.same_f32(root, zp["root_box"])


# ---- ray_march ---------------------------------------------------------------------------
def test_ray_march_batch(tree, zm):
    _same_march(tree.ray_march(zm["batch_rays"]), zm, "batch_")
    _same_march(tree.ray_march(zm["film_rays"]), zm, "film_")
    # a scene without probes: even_invisible changes nothing
    _same_march(tree.ray_march(zm["batch_rays"], even_invisible=True), zm, "batch_")


@pytest.mark.parametrize("on_device", [False, True], ids=["host_build", "device_build"])
def test_probe_scene_march(sd, zp, on_device):
    p = vrt.VoxelOctree(sd, int(zp["probe_depth"]), build_on_device=on_device, probes=zp["scene_probes"])
    _same_march(p.ray_march(zp["rays"], even_invisible=True), zp, "even_")
    _same_march(p.ray_march(zp["rays"], even_invisible=False), zp, "visible_")
    on_probe = (zp["even_hit"] == 1) & (zp["even_tri"] >= sd.ntri)
    assert on_probe.sum() >= 100


def test_primary_render_samples(tree, zm):
    rgb, so = tree.render(vrt.Camera(*rec.cam_of(zm["cam"])), _film(zm), samples=True)
    assert np.array_equal(so["hit"], zm["film_hit"])
    assert np.array_equal(so["tri"], zm["film_tri"]) and np.array_equal(so["voxel"], zm["film_voxel"])
    hit = zm["film_hit"] == 1
    assert rc.same_f32(so["rgb"][hit], zm["film_diffuse"][hit]), rc.diff_count(so["rgb"][hit], zm["film_diffuse"][hit])
    assert rc.same_f32(so["rgb"][~hit], rc.sky(zm["film_rays"])[~hit])
    assert rc.same_f32(rgb, zm["film_image"])


# ---- the light map --------------------------------------------------------------------------
def test_lightmap_nodes(lit, zm, zl):
    key, cov, ill = lit.lightmap_nodes()
    assert np.array_equal(key, zm["node_key"])
    assert rc.same_f32(cov, zl["white_cov"]), rc.diff_count(cov, zl["white_cov"])
    want = rec.illum_of(zl, "white")
    assert rc.same_f32(ill, want), rc.diff_count(ill, want)


def test_lightmap_lights_nodes(sd, zm, zl):
    t = vrt.VoxelOctree(sd, int(zl["depth"]))
    lights = [vrt.Light(vrt.Camera(*rec.cam_of(zl[f"light{i}_cam"])), _light_film(zl), zl[f"light{i}_color"])
              for i in range(2)]
    assert t.lightmap_lights(lights) == int(zl["lights_hits"].sum())
    key, cov, ill = t.lightmap_nodes()
    assert np.array_equal(key, zm["node_key"])
    assert rc.same_f32(cov, zl["lights_cov"])
    want = rec.illum_of(zl, "lights")
    assert rc.same_f32(ill, want), rc.diff_count(ill, want)
    # one light of the list alone is the white map
    assert t.lightmap_lights(lights[:1]) == int(zl["white_hits"])
    assert rc.same_f32(t.lightmap_nodes()[2], rec.illum_of(zl, "white"))


# ---- cone_trace and trace() --------------------------------------------------------------------
def _min_voxel(zl, tag):
    return float(zl["res"]) if tag == "res" else 0.01


@pytest.mark.parametrize("tag", rec.MIN_VOXELS)
def test_cone_trace_and_trace_batch(lit, zm, zl, tag):
    mv = _min_voxel(zl, tag)
    assert lit.min_voxel(6) == float(zl["res"])
    hit = zm["film_hit"] == 1
    want = zl[f"film_indirect_{tag}"]
    got = lit.cone_trace(zm["film_hit_p"][hit], zm["film_normal"][hit], mv)
    assert rc.same_f32(got, want[hit]), rc.diff_count(got, want[hit])
    rgb, parts = lit.trace(zm["film_rays"], mv, parts=True)
    assert np.array_equal(parts["hit"], zm["film_hit"]) and np.array_equal(parts["tri"], zm["film_tri"])
    assert rc.same_f32(parts["indirect"], want)
    assert rc.same_f32(parts["direct"], zl["film_direct"])
    assert rc.same_f32(parts["albedo"], zm["film_albedo"])
    assert rc.same_f32(rgb, zl[f"film_trace_{tag}"]), rc.diff_count(rgb, zl[f"film_trace_{tag}"])


@pytest.mark.parametrize("tag", rec.MIN_VOXELS)
def test_trace_frame_one_call(sd, zm, zl, tag):
    import torch
    t = vrt.VoxelOctree(sd, int(zl["depth"]))
    film = _film(zm)
    img = torch.zeros((film.ny, film.nx, 3), device="cuda")
    torch.cuda.synchronize()
    hits = t.trace_frame_device(vrt.Camera(*rec.cam_of(zl["light0_cam"])), _light_film(zl),
                                vrt.Camera(*rec.cam_of(zm["cam"])), film, 0, 1, 1, img.data_ptr(),
                                _min_voxel(zl, tag))
    torch.cuda.synchronize()
    assert hits == int(zl["white_hits"])
    got, want = img.cpu().numpy(), zl[f"film_image_{tag}"]
    assert rc.same_f32(got, want), rc.diff_count(got.reshape(-1, 3), want.reshape(-1, 3))
    # and the host-array frame on the lit scene
    assert rc.same_f32(t.render_trace(vrt.Camera(*rec.cam_of(zm["cam"])), film, _min_voxel(zl, tag)), want)


# ---- light probes ---------------------------------------------------------------------------------
def test_probe_gather_and_eval(lit, zp):
    import torch
    got = lit.probe_gather(zp["gather_probes"], float(zp["res"]), zp["light_color"])
    assert rc.same_f32(got["a"], zp["sg_a"]), rc.diff_count(got["a"].reshape(-1, 3), zp["sg_a"].reshape(-1, 3))
    assert rc.same_f32(got["d"], zp["sg_d"]) and rc.same_f32(got["s"], zp["sg_s"])
    sgs = {"a": zp["sg_a"], "d": zp["sg_d"], "s": zp["sg_s"]}
    dirs = zp["eval_dirs"]
    ev = vrt.probe_eval(sgs, dirs)
    assert rc.same_f32(ev, zp["eval"]), rc.diff_count(ev.reshape(-1, 3), zp["eval"].reshape(-1, 3))
    n, m = len(zp["sg_a"]), len(dirs)
    recs = np.ascontiguousarray(np.concatenate([sgs["a"], sgs["d"], sgs["s"][:, :, None]], axis=2))
    d_sgs, d_dirs = torch.from_numpy(recs).cuda(), torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    d_rgb = torch.full((n, m, 3), 7.0, device="cuda")
    torch.cuda.synchronize()
    vrt.probe_eval_device(d_sgs.data_ptr(), n, d_dirs.data_ptr(), m, d_rgb.data_ptr())
    torch.cuda.synchronize()
    assert rc.same_f32(d_rgb.cpu().numpy(), zp["eval"])
