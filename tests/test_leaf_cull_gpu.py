"""GPU tests of the leaf-record cull (leaf_isect_cull, vrt_kernels.hip): small
frames of the flagship scene through the production launch, and a synthetic
soup whose one crowded leaf spans three 32-record blocks, with rays aimed at
the block seams, at exact ties and past every record box -- all against the
oracle's ray_march."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ frames
@pytest.fixture(scope="module")
def proxy8():
    sd = vrt.SceneData.proxy(1.0, 1)
    return sd, vrt.VoxelOctree(sd, 8), po.Scene(sd, 8)


def _cameras(tree):
    """Pose 0 of the sweep, and pose 5 sheared so that d_y = 0.75 x - y / 64
    (s.y = 0.75, u.y = -1/64, nf.y = 0) cancels exactly on six sample-1 rays
    of a 256x144 film (x = (8 (px - 128) + 3) / 2048 and y = (8 (71 - py) +
    1) / 1152 meet at py = 61 - 27 k, px = 128 + k): those units are deferred
    to k_render_defer, the others take the fast-only kernel."""
    mn, mx = tree.root_box
    out = []
    for pose, shear in ((0, None), (5, {1: 0.75, 5: -1.0 / 64, 9: 0.0})):
        fov, eye, spot, up = vrt.sweep_pose(mn, mx, pose, 16)
        cam, ocam = vrt.Camera(fov, eye, spot, up), po.camera(fov, eye, spot, up)
        for k, v in (shear or {}).items():
            cam.c.C[k] = v
            ocam[k] = v
        out.append((cam, ocam))
    return out


def test_small_frames_equal_the_oracle(proxy8):
    """256x144 at depth 8 through vrt_render_tiles_device (k_render_p<true>
    with the cull; k_render_defer for the camera that defers units): both
    cameras one launch each, then three frames in flight on three streams.
    Film bits equal the oracle's."""
    import torch
    sd, tree, osc = proxy8
    assert tree.ref_record_bytes == 48
    film = vrt.Film(1, 1, 256, 144)
    cams = _cameras(tree)
    assert cams[0][0].defer_bound(film) == 0 and cams[1][0].defer_bound(film) > 0
    dev = torch.device("cuda:0")
    want = []
    for cam, ocam in cams:
        want.append(osc.render(ocam, 1.0, 1.0, 256, 144, film_index=1, nthreads=16, samples=False))
        img = torch.zeros((144, 256, 3), dtype=torch.float32, device=dev)
        tree.render_tiles_device(cam, film, 0, 1, 1, img.data_ptr(), None)
        torch.cuda.synchronize()
        assert np.array_equal(bits(img.cpu().numpy()), bits(want[-1])), len(want) - 1
    # 3 frames in flight (smaller persistent grids, one queue slot per stream)
    tree.set_frames_in_flight(3)
    try:
        streams = [torch.cuda.Stream(dev) for _ in range(3)]
        seq = [0, 1, 0]
        imgs = [torch.zeros((144, 256, 3), dtype=torch.float32, device=dev) for _ in seq]
        torch.cuda.synchronize()
        for ci, img, st in zip(seq, imgs, streams):
            tree.render_tiles_device(cams[ci][0], film, 0, 1, 1, img.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        for ci, img in zip(seq, imgs):
            assert np.array_equal(bits(img.cpu().numpy()), bits(want[ci])), ("in flight", ci)
    finally:
        tree.set_frames_in_flight(1)


# ------------------------------------------------- block seams and order
NTILE = 70           # records 0..69 of the crowded leaf: small tiles in the plane z ~ 0.40
WALL = NTILE         # record 70, the leaf's last: a wall behind half of the tiles
DUP = {40: 10, 66: 33}  # record -> the earlier record it duplicates (another id, same vertices)
TARGET = WALL + 1    # a triangle in a later leaf along +x
DEPTH = 4            # leaf voxels of 1/8 over the unit root box; the crowded one is [0.375, 0.5]^3


def _slot(k):
    k = DUP.get(k, k)
    return 0.385 + 0.0115 * (k % 9), 0.385 + 0.0115 * (k // 9)


def _tile_z(k):
    return 0.40 + 0.0002 * (DUP.get(k, k) % 7)


def _soup():
    tris = []
    for k in range(NTILE):
        cx, cy = _slot(k)
        z = _tile_z(k)
        tris.append([cx - 0.004, cy - 0.004, z, cx + 0.004, cy - 0.004, z, cx, cy + 0.004, z])
    tris.append([0.378, 0.378, 0.48, 0.498, 0.378, 0.48, 0.378, 0.498, 0.48])  # WALL
    tris.append([0.7, 0.38, 0.38, 0.7, 0.495, 0.38, 0.7, 0.44, 0.495])          # TARGET
    # the root box's corners, and single-triangle leaves far behind (z = 0.78)
    tris.append([0, 0, 0, 0.05, 0, 0, 0, 0.05, 0])
    tris.append([1, 1, 1, 0.95, 1, 1, 1, 0.95, 1])
    for i in range(30):
        x, y, z = (i % 8) / 8 + 0.03, (i // 8) / 8 + 0.03, 0.78
        tris.append([x, y, z, x + 0.05, y, z, x, y + 0.05, z])
    pos = np.array(tris, F)
    return vrt.SceneData(pos, np.tile(F([0, 0, -1]), (len(pos), 3)))


def _rays(origin):
    """Rays from one origin at every tile (a point inside it), at gaps
    between tiles over the wall, and the ray that runs between the tile plane
    and the wall; none has a zero direction component (the finite-slab walk)."""
    tg = [(_slot(k)[0], _slot(k)[1] - 0.001, _tile_z(k)) for k in range(NTILE)]
    tg += [(0.39075 + 0.0115 * i, 0.39075, 0.401) for i in range(4)]  # gaps between tiles: the wall alone
    rays = [vrt.make_ray(origin, np.float64(t) - np.float64(origin)) for t in tg]
    rays.append(vrt.make_ray((-0.3, 0.435, 0.445), (1.0, 0.005, -0.005)))
    rays = np.array(rays, F)
    assert np.all(rays[:, 3:6] != 0)
    return rays


@pytest.fixture(scope="module")
def seams():
    sd = _soup()
    tree, osc = vrt.VoxelOctree(sd, DEPTH), po.Scene(sd, DEPTH)
    return sd, tree, osc


def test_crowded_leaf_selects_the_48_byte_format(seams):
    sd, tree, osc = seams
    assert tree.ref_record_bytes == 48
    vox, cnt, tris = tree.leaves()
    k = int(np.argmax(cnt))
    assert cnt[k] == WALL + 1 >= 65
    first = int(np.sum(cnt[:k]))
    assert list(tris[first:first + cnt[k]]) == list(range(WALL + 1))  # records in input order
    assert np.allclose(tree.root_box[0], 0) and np.allclose(tree.root_box[1], 1)


@pytest.mark.parametrize("origin", [(0.4507, 0.4337, -0.6), (0.4507, 0.4337, -20.0)], ids=["near", "beyond_lb_reach"])
def test_block_seams_ties_and_misses(seams, origin):
    """Nearest hit at record 0, 31, 32, 64 and the last record; exact ties
    between a record and its duplicate in a later block give the lower
    index; a ray that meets no record box of the crowded leaf goes on to a
    later leaf.  From the near origin the wave culls; from beyond lb_reach
    (16 x the extent from the centre) nothing is culled.  Hit, triangle,
    voxel -- and the hit point and normal bits -- equal the oracle's."""
    sd, tree, osc = seams
    rays = _rays(origin)
    want = osc.ray_march(rays)
    # the oracle confirms the rays exercise what they are aimed at
    for k in (0, 31, 32, 64):
        assert want["hit"][k] and want["tri"][k] == k
    for k, lower in DUP.items():
        assert want["tri"][k] == lower and want["tri"][lower] == lower  # the tie goes to the lower index
    assert np.all(want["tri"][NTILE:NTILE + 4] == WALL)                  # the leaf's last record alone
    assert want["tri"][-1] == TARGET and want["counters"][-1, 2] >= WALL + 1  # walked the crowded leaf, hit later
    assert np.all(want["hit"] == 1)
    got = tree.ray_march(rays)
    for key in ("hit", "tri", "voxel"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(bits(got["hit_p"]), bits(want["hit_p"]))
    assert np.array_equal(bits(got["normal"]), bits(want["normal"]))
