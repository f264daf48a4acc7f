"""The recorded-reference fixtures tests/golden/ref_gi_*.npz: what they hold,
how the reference library computes them (record(), called by
tests/golden/make_golden.py and, where the reference runs, by
test_recorded_reference_is_current), and the oracle's check against them
(check_oracle(), which needs no reference and no GPU).

Only data is recorded: the inputs (cameras, films, ray batches, lights,
probes; the scene itself is the committed scene_proxy.npz, named by its
SHA-256) and the outputs of the reference's own compiled camera.cc /
voxel_octree.cc.  A helper module: it holds no tests."""
import hashlib
import os

import numpy as np

import pyoracle as po
import voxelraytrace20190722_amd as vrt

import lights_model as lm
import probe_cases as pc
import probe_scene_cases as psc
import reference_gi_cases as rc

F = np.float32
DEPTH = 6          # the triangle scene
PROBE_DEPTH = 5    # the probe scene
FILM = (1.0, 1.0, 32, 32)
LIGHT_N = 128
NBATCH = 2048
NPROBE_RAYS = 1024
MIN_VOXELS = ("res", "p01")  # the scene's own Res (6 levels) and 0.01


def scene():
    z = np.load(os.path.join(rc.GOLDEN, "scene_proxy.npz"), allow_pickle=False)
    return rc.scene_from(z)


def scene_sha(sd):
    h = hashlib.sha256()
    for k, v in sorted(rc.scene_arrays(sd).items()):
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return np.array(h.hexdigest())


def cam_arr(cam):
    return np.array([cam[0], *cam[1], *cam[2], *cam[3]], F)


def cam_of(a):
    return (float(a[0]), tuple(float(v) for v in a[1:4]), tuple(float(v) for v in a[4:7]),
            tuple(float(v) for v in a[7:10]))


def lights():
    return [lm.ModelLight(rc.LIGHT, (LIGHT_N, LIGHT_N)), lm.ModelLight(rc.LIGHT2, (LIGHT_N, LIGHT_N), rc.COLOR2)]


def sparse(a):
    """Rows of a that are not all +0 -> (indices, rows)."""
    flat = a.reshape(len(a), -1)
    idx = np.flatnonzero((flat.view(np.uint32) != 0).any(axis=1)).astype(np.int32)
    return idx, np.ascontiguousarray(a[idx])


def dense(n, idx, rows):
    out = np.zeros((n,) + rows.shape[1:], rows.dtype)
    out[idx] = rows
    return out


def _march_rec(prefix, r, rec, pieces=("diffuse", "albedo")):
    rec[prefix + "hit"] = r["hit"].astype(np.int8)
    rec[prefix + "tri"] = r["tri"]
    rec[prefix + "voxel"] = r["voxel"]
    for k in ("hit_p", "normal") + tuple(pieces):
        rec[prefix + k] = r[k]


def record(texdir):
    """-> {fixture name: {key: array}} from the reference library."""
    sd = scene()
    names = rc.texture_files(sd, texdir, "scene_proxy")
    sha = scene_sha(sd)
    out = {}

    # ---- march: the tree, a film's samples, a ray batch --------------------------------
    ref = po.RefScene(sd, DEPTH, texnames=names)
    m = {"scene_sha": sha, "depth": np.int32(DEPTH), "cam": cam_arr(rc.VIEW), "film": np.array(FILM, F)}
    m["leaf_voxel"], m["leaf_count"], m["leaf_list"] = ref.leaves()
    key, box = ref.boxes()
    m["root_box"] = box[0]
    m["node_key"] = key
    film_rays = po.ref_gen_rays(rc.VIEW, *FILM).reshape(-1, 8)
    m["film_rays"] = film_rays
    white = ref.ray_march(film_rays, even_invisible=True, pieces=True)
    _march_rec("film_", white, m)
    # the primary render's film: get_diffuse under white (the sky on a miss), Film::add(c * .25f)
    prim = np.where((white["hit"] == 1)[:, None], white["diffuse"], rc.sky(film_rays)).astype(F)
    m["film_image"] = po.ref_film_add(*FILM, rc.film_samples(FILM[2], FILM[3]), (prim * F(0.25)).astype(F))
    batch = rc.batch_rays(606, NBATCH, box[0, :3], box[0, 3:])
    m["batch_rays"] = batch
    _march_rec("batch_", ref.ray_march(batch, pieces=True), m)
    out["march"] = m

    # ---- light: node records of two light maps, cones, trace() and its film ----------------
    L = {"scene_sha": sha, "depth": np.int32(DEPTH), "light_n": np.int32(LIGHT_N)}
    ls = lights()
    for i, l in enumerate(ls):
        L[f"light{i}_cam"], L[f"light{i}_color"] = cam_arr(l.cam), np.array(l.color, F)
    both = po.RefScene(sd, DEPTH, texnames=names)
    L["lights_hits"] = np.array([both.lightmap(l.cam, 1.0, 1.0, LIGHT_N, LIGHT_N, color=l.color, filter=False)
                                 for l in ls], np.int64)
    both.filter()
    L["white_hits"] = np.int64(ref.lightmap(ls[0].cam, 1.0, 1.0, LIGHT_N, LIGHT_N))
    for name, s in (("white", ref), ("lights", both)):
        k, cov, ill = s.lightmap_nodes()
        assert np.array_equal(k, key)
        L[name + "_cov"] = cov
        L[name + "_illum_at"], L[name + "_illum"] = sparse(ill)
    res = ref.min_voxel(6)
    L["res"] = F(res)
    lit = ref.ray_march(film_rays, even_invisible=True, pieces=True)
    hit = lit["hit"] == 1
    L["film_direct"] = lit["illum"]
    for tag, mv in zip(MIN_VOXELS, (res, 0.01)):
        ind = np.zeros((len(film_rays), 3), F)
        ind[hit] = ref.cone_trace(lit["hit_p"][hit], lit["normal"][hit], mv)
        L[f"film_indirect_{tag}"] = ind
        rgb = rc.combine_trace(film_rays, lit["hit"], lit["visible"], lit["albedo"], ind, lit["illum"])
        L[f"film_trace_{tag}"] = rgb
        L[f"film_image_{tag}"] = po.ref_film_add(*FILM, rc.film_samples(FILM[2], FILM[3]), (rgb * F(0.25)).astype(F))
    out["light"] = L

    # ---- probes: gather and eval on the lit scene; a probe scene's tree and marches --------------
    P = {"scene_sha": sha, "depth": np.int32(DEPTH), "probe_depth": np.int32(PROBE_DEPTH), "res": F(res),
         "light_color": np.array(rc.PROBE_LIGHT, F), "light_cam": cam_arr(rc.LIGHT), "light_n": np.int32(LIGHT_N)}
    gp = rc.scene_probes(box[0, :3], box[0, 3:], n=4, seed=21)
    P["gather_probes"] = gp
    sg = ref.probe_gather(gp, res, rc.PROBE_LIGHT)
    P["sg_a"], P["sg_d"], P["sg_s"] = sg["a"], sg["d"], sg["s"]
    dirs = rc.unit_dirs(8, 256)
    P["eval_dirs"] = dirs
    P["eval"] = np.stack([po.ref_probe_eval(np.concatenate([sg["a"][k], sg["d"][k], sg["s"][k][:, None]], axis=1), dirs)
                          for k in range(len(gp))])
    sp = rc.scene_probes(box[0, :3], box[0, 3:], n=8)
    P["scene_probes"] = sp
    pref = po.RefScene(sd, PROBE_DEPTH, probes=sp, texnames=names)
    P["leaf_voxel"], P["leaf_count"], P["leaf_list"] = pref.leaves()
    pkey, pbox = pref.boxes()
    P["node_key"], P["root_box"] = pkey, pbox[0]
    rays = probe_scene_rays(sp, pbox[0, :3], pbox[0, 3:])
    P["rays"] = rays
    _march_rec("even_", pref.ray_march(rays, even_invisible=True), P, pieces=())
    _march_rec("visible_", pref.ray_march(rays, even_invisible=False), P, pieces=())
    out["probes"] = P
    return out


def probe_scene_rays(probes, mn, mx):
    """Rays aimed at and near the probes from around the scene, and random ones."""
    rng = np.random.default_rng(3)
    n = NPROBE_RAYS * 5 // 8
    org = (mn + rng.uniform(-0.2, 1.2, (n, 3)) * (mx - mn)).astype(F)
    tgt = probes[rng.integers(0, len(probes), n), :3] + rng.normal(0, 0.05, (n, 3)).astype(F)
    aimed = np.stack([po.make_ray(a, b - a, 0.0, rc.FLT_MAX) for a, b in zip(org, tgt)])
    return np.ascontiguousarray(np.concatenate([aimed, rc.random_rays(rng, NPROBE_RAYS - n, mn, mx)]))


def save(texdir):
    """Write the fixtures; returns {file: bytes}."""
    sizes = {}
    for name, rec in record(texdir).items():
        path = os.path.join(rc.GOLDEN, f"ref_gi_{name}.npz")
        np.savez_compressed(path, **rec)
        sizes[os.path.basename(path)] = os.path.getsize(path)
    return sizes


def split_leaves(voxel, count, lst, ntri):
    """A mixed tree's leaves -> (triangle leaves, probe leaves), each as
    (voxel, count, list) with probe k named k, as vrt_scene_leaves and
    vrt_scene_probe_leaves give them."""
    off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    lists = [lst[off[i]:off[i + 1]] for i in range(len(voxel))]

    def side(sel, shift):
        ls = [l[sel(l)] - shift for l in lists]
        keep = np.array([len(l) > 0 for l in ls], bool)
        cat = np.concatenate([l for l in ls if len(l)]) if keep.any() else np.zeros(0, np.int32)
        return voxel[keep], np.array([len(l) for l in ls if len(l)], np.uint32), cat.astype(np.int32)
    return side(lambda l: l < ntri, 0), side(lambda l: l >= ntri, ntri)


def illum_of(z, name):
    return dense(len(z[name + "_cov"]), z[name + "_illum_at"], z[name + "_illum"])


# ---- the oracle against the fixtures --------------------------------------------------------
def check_oracle(golden):
    sd = scene()
    m, L, P = (golden(f"ref_gi_{n}.npz") for n in ("march", "light", "probes"))
    sha = scene_sha(sd)
    assert str(m["scene_sha"]) == str(L["scene_sha"]) == str(P["scene_sha"]) == str(sha)
    depth = int(m["depth"])
    osc = po.Scene(sd, depth)
    # tree
    for a, k in zip(osc.leaves(), ("leaf_voxel", "leaf_count", "leaf_list")):
        assert np.array_equal(a, m[k]), k
    key, box = osc.boxes()
    assert np.array_equal(key, m["node_key"]) and rc.same_f32(box[0], m["root_box"])
    # camera
    film = m["film"]
    fw, fh, nx, ny = float(film[0]), float(film[1]), int(film[2]), int(film[3])
    cam = cam_of(m["cam"])
    rays = rc.oracle_film_rays(cam, fw, fh, nx, ny).reshape(-1, 8)
    assert rc.same_f32(rays, m["film_rays"])
    # marches and pieces
    for pre, r in (("film_", rays), ("batch_", m["batch_rays"])):
        o = osc.ray_march(r)
        p = osc.hit_pieces(r)
        assert np.array_equal(o["hit"], m[pre + "hit"]), pre
        assert np.array_equal(o["tri"], m[pre + "tri"]) and np.array_equal(o["voxel"], m[pre + "voxel"]), pre
        for k in ("hit_p", "normal"):
            assert rc.same_f32(o[k], m[pre + k]), (pre, k)
        for k in ("diffuse", "albedo"):
            assert rc.same_f32(p[k], m[pre + k]), (pre, k)
    img = osc.render(po.camera(*cam), fw, fh, nx, ny, film_index=1, nthreads=8, samples=False)
    assert rc.same_f32(img, m["film_image"])
    assert 1000 < int(m["film_hit"].sum()) < len(rays) and 100 < int(m["batch_hit"].sum()) < NBATCH
    # light maps: the oracle's own for the white light, the light-list model for both
    n = int(L["light_n"])
    ls = [lm.ModelLight(cam_of(L[f"light{i}_cam"]), (n, n), tuple(float(c) for c in L[f"light{i}_color"]))
          for i in range(2)]
    mh, (mkey, mcov, mill) = lm.lightmap(osc, ("ref_gi_fixture", depth), ls)
    assert mh == int(L["lights_hits"].sum()) and np.array_equal(mkey, key)
    assert rc.same_f32(mcov, L["lights_cov"]) and rc.same_f32(mill, illum_of(L, "lights"))
    assert osc.lightmap(po.camera(*ls[0].cam), 1.0, 1.0, n, n, nthreads=8) == int(L["white_hits"])
    okey, ocov, oill = osc.lightmap_nodes()
    assert np.array_equal(okey, key) and rc.same_f32(ocov, L["white_cov"]) and rc.same_f32(oill, illum_of(L, "white"))
    # cones, trace() and its film on the white map
    res = float(L["res"])
    assert res == osc.min_voxel(6)
    hit = m["film_hit"] == 1
    assert rc.same_f32(osc.hit_pieces(rays)["illum"], L["film_direct"])
    for tag, mv in zip(MIN_VOXELS, (res, 0.01)):
        ind = L[f"film_indirect_{tag}"]
        assert rc.same_f32(osc.cone_trace(m["film_hit_p"][hit], m["film_normal"][hit], mv), ind[hit]), tag
        assert rc.same_f32(osc.shade_trace(rays, mv), L[f"film_trace_{tag}"]), tag
        img = osc.render_trace(po.camera(*cam), fw, fh, nx, ny, mv, samples=False)
        assert rc.same_f32(img, L[f"film_image_{tag}"]), tag
    # probes: gather_light and eval restated on the oracle
    gp = P["gather_probes"]
    pr = pc.probe_rays(gp, po.sphere_points(pc.SEED, 100), res)
    h = osc.ray_march(pr)
    ph = h["hit"] == 1
    terms = np.tile(P["light_color"], (len(pr), 1))
    terms[ph] = osc.cone_trace(h["hit_p"][ph], h["normal"][ph], res)
    assert rc.same_f32(pc.seq_sum_div(terms.reshape(len(gp), 14, 100, 3)), P["sg_a"])
    assert rc.same_f32(np.tile(pc.normalize(pc.DIRS), (len(gp), 1, 1)), P["sg_d"])
    assert np.all(rc.bits(P["sg_s"]) == rc.bits(F(10)))
    assert rc.same_f32(pc.eval_restated(P["sg_a"], P["sg_d"], P["sg_s"], P["eval_dirs"]), P["eval"])
    # the probe scene: the product's host build and the restated mixed walk over it
    sp, pdepth = P["scene_probes"], int(P["probe_depth"])
    tree = vrt.VoxelOctree(sd, pdepth, device=-1, probes=sp)
    tl, pl = split_leaves(P["leaf_voxel"], P["leaf_count"], P["leaf_list"], sd.ntri)
    for got, want in ((tree.leaves(), tl), (tree.probe_leaves(), pl)):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    bx, wa, wtl, wpl = psc.tree_lists(tree)
    keys = pc.node_keys(wa)
    assert np.array_equal(np.sort(keys), P["node_key"]) and rc.same_f32(bx[0], P["root_box"])
    walker = psc.Walker(sd, sp, bx, wa, wtl, wpl, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    pick = np.concatenate([np.arange(0, 160), np.arange(NPROBE_RAYS - 80, NPROBE_RAYS)])
    for pre, even in (("even_", True), ("visible_", False)):
        w = walker.batch(P["rays"][pick], even_invisible=even)
        assert np.array_equal(w["hit"], P[pre + "hit"][pick]), pre
        assert np.array_equal(w["tri"], P[pre + "tri"][pick]) and np.array_equal(w["voxel"], P[pre + "voxel"][pick])
        assert rc.same_f32(w["hit_p"], P[pre + "hit_p"][pick]) and rc.same_f32(w["normal"], P[pre + "normal"][pick])
    on_probe = (P["even_hit"] == 1) & (P["even_tri"] >= sd.ntri)
    assert on_probe.sum() >= 100 and not ((P["visible_hit"] == 1) & (P["visible_tri"] >= sd.ntri)).any()
