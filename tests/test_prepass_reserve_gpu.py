"""GPU tests of the grid of one-rank frames in flight that take the beam entry
(launch_render, vrt_kernels.hip).  Such a frame launches its
persistent grid -- and its deferred pass -- on its share of the block slots;
block slots left free for the other frames' pre-passes (a "pre-pass reserve")
were measured and not kept, and these tests hold for any such grid: the work
queue's bases are counted from the grid actually launched, so a wrong count
shows as a wrong image once a ring slot is reused.  Small frames through the
production launch on three streams, more than two turns of the 8-slot ring,
bit for bit against the oracle and against the same pose rendered with one
frame in flight."""
import numpy as np
import pytest

import pyoracle as po
import voxelraytrace20190722_amd as vrt

pytestmark = pytest.mark.gpu

DETAIL, DEPTH = 0.02, 6  # 48-B leaf records: the production launch is k_render_p<true>
POSES = (0, 5, 9, 13)
NX, NY = 320, 200  # 1,000 tiles: more than a frame's share of the slots with frames in flight
FRAMES = 20


@pytest.fixture(autouse=True)
def small_frames_take_the_entry():
    """The tests' frames are far below kEntryMinUnits."""
    old = vrt.test_flags()
    vrt.set_test_flags(old | vrt.TEST_SMALL_BEAM_ENTRY)
    yield
    vrt.set_test_flags(old)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    def __init__(self):
        sd = vrt.SceneData.proxy(DETAIL, 1)
        self.tree = vrt.VoxelOctree(sd, DEPTH)
        assert self.tree.ref_record_bytes == 48
        self.osc = po.Scene(sd, DEPTH)
        mn, mx = self.tree.root_box
        self.poses = {k: vrt.sweep_pose(mn, mx, k, 16) for k in POSES}
        self._want = {}

    def want(self, pose, nx=NX, ny=NY):
        """The oracle's image, computed once per (pose, film)."""
        key = (pose, nx, ny)
        if key not in self._want:
            self._want[key] = self.osc.render(po.camera(*self.poses[pose]), 1.0, 1.0, nx, ny, film_index=1,
                                              nthreads=16, samples=True)[0]
        return self._want[key]

    def one(self, pose, nx=NX, ny=NY):
        """One frame alone on torch's stream."""
        import torch
        img = torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        self.tree.render_tiles_device(vrt.Camera(*self.poses[pose]), vrt.Film(1, 1, nx, ny), 0, 1, 1, img.data_ptr(),
                                      None)
        torch.cuda.synchronize()
        assert self.tree.beam_entries() is not None  # the frame took the entry
        return img.cpu().numpy()

    def in_flight(self, n, nx=NX, ny=NY):
        """n consecutive frames over the poses on three streams."""
        import torch
        film = vrt.Film(1, 1, nx, ny)
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda:0") for _ in range(n)]
        torch.cuda.synchronize()  # the zero fills ran on torch's stream
        for k in range(n):
            self.tree.render_tiles_device(vrt.Camera(*self.poses[POSES[k % len(POSES)]]), film, 0, 1, 1,
                                          outs[k].data_ptr(), streams[k % 3].cuda_stream)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]


@pytest.fixture(scope="module")
def case():
    return Case()


@pytest.fixture(scope="module")
def alone(case):
    """Every pose rendered with one frame in flight (the whole grid)."""
    old = vrt.test_flags()
    vrt.set_test_flags(old | vrt.TEST_SMALL_BEAM_ENTRY)
    try:
        return {k: case.one(k) for k in POSES}
    finally:
        vrt.set_test_flags(old)


def test_twenty_frames_in_flight(case, alone):
    """20 frames, 3 in flight: every one equals the oracle's image and the
    one-frame-in-flight render of its pose; then one more frame after the hint
    is reset."""
    for k in POSES:
        assert np.array_equal(bits(alone[k]), bits(case.want(k))), k
    case.tree.set_frames_in_flight(3)
    try:
        got = case.in_flight(FRAMES)
    finally:
        case.tree.set_frames_in_flight(1)
    for k, g in enumerate(got):
        pose = POSES[k % len(POSES)]
        assert np.array_equal(bits(g), bits(case.want(pose))), k
        assert np.array_equal(bits(g), bits(alone[pose])), k
    assert np.array_equal(bits(case.one(5)), bits(case.want(5)))


def test_twenty_deferred_frames_in_flight(case, alone):
    """The same with every unit deferred: k_render_defer on the frame's grid,
    from the slices' lists (500 units per slice at 320x200, within
    kDeferSliceCap = 512) and, at 352x208 (572 per slice), re-rendering whole
    slices."""
    old = vrt.test_flags()
    case.tree.set_frames_in_flight(3)
    try:
        vrt.set_test_flags(old | vrt.TEST_FORCE_DEFER)
        got = case.in_flight(FRAMES)
        big = case.in_flight(len(POSES), 352, 208)
    finally:
        vrt.set_test_flags(old)
        case.tree.set_frames_in_flight(1)
    for k, g in enumerate(got):
        pose = POSES[k % len(POSES)]
        assert np.array_equal(bits(g), bits(case.want(pose))), k
        assert np.array_equal(bits(g), bits(alone[pose])), k
    for k, g in enumerate(big):
        assert np.array_equal(bits(g), bits(case.want(POSES[k], 352, 208))), k
    # the counts were reset: a normal frame on the same ring renders fully
    assert np.array_equal(bits(case.one(9)), bits(case.want(9)))


def test_film_smaller_than_the_reserve(case):
    """A 64x48 film needs 48 blocks, fewer than a frame's share of the slots
    (and than any reserve): the grid is the film's own, with and without
    frames in flight."""
    case.tree.set_frames_in_flight(3)
    try:
        got = case.in_flight(4, 64, 48)
    finally:
        case.tree.set_frames_in_flight(1)
    for k, g in enumerate(got):
        assert np.array_equal(bits(g), bits(case.want(POSES[k], 64, 48))), k
    assert np.array_equal(bits(case.one(0, 64, 48)), bits(case.want(0, 64, 48)))
