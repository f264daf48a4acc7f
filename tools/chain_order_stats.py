#!/usr/bin/env python3
"""Host estimate of how often the chain order falls back to
the sort on the bench's frames; no GPU.  For sampled units (4x4 pixels x 4
samples = one wave) of every sweep pose at 1080p, depth 8: the fraction of
units in which some ray fails the per-ray criterion (the whole walk sorts),
and, among the units that pass, the fraction of wave expansions with >= 2 hit
children in some lane where some lane's hit set is no chain (that expansion
sorts).  The walk here visits every hit child of every hit node (no early
exit at the first triangle, no triangle-box skip), a superset of the
kernel's visits.

usage: tools/chain_order_stats.py [--units 200] [--poses 16]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxelraytrace20190722_amd as vrt  # noqa: E402
import pyoracle as po  # noqa: E402
import chain_order_cases as cc  # noqa: E402

F = np.float32
LEAF = np.uint32(0x80000000)


def spacing(box, a):
    """vrt_host.cpp's chain_spacing over a tree's internal nodes."""
    inner = (a & LEAF) == 0
    a0, b, c = cc.planes(box[inner, :3], box[inner, 3:])
    w = ((b + c) * F(.5)).astype(np.float64) - ((a0 + b) * F(.5)).astype(np.float64)
    w = w.min(0)
    f = w.astype(F)
    f = np.where(f.astype(np.float64) > w, np.nextafter(f, F(0)), f)
    return f.astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=200)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    a = ap.parse_args()
    sd = vrt.SceneData.proxy(1.0, 1)
    tree = vrt.VoxelOctree(sd, a.depth, device=-1)
    box, wa, wb = tree.nodes()
    mn, mx = tree.root_box
    wmin = spacing(box, wa)
    rng = np.random.default_rng(1)
    tot = {"units": 0, "units_fail": 0, "exp": 0, "exp_order": 0, "exp_nonchain": 0}
    for pose in range(a.poses):
        fov, eye, spot, up = vrt.sweep_pose(mn, mx, pose, a.poses)
        cam = po.camera(fov, eye, spot, up)
        ux = rng.integers(0, a.width // 4, a.units)
        uy = rng.integers(0, a.height // 4, a.units)
        rays = []
        for x, y in zip(ux, uy):
            for p in range(16):
                rays.append(po.gen_rays4(cam, 1.0, 1.0, a.width, a.height, int(4 * x + p % 4), int(4 * y + p // 4)))
        rays = np.asarray(rays, F).reshape(-1, 8)
        o, d = rays[:, :3], rays[:, 3:6]
        unit = np.repeat(np.arange(a.units), 64)
        n = len(o)
        crit = cc.criterion(np.tile(mn, (n, 1)), np.tile(mx, (n, 1)), o, d, wmin)
        ok_unit = np.logical_and.reduceat(crit, np.arange(0, n, 64))
        tot["units"] += a.units
        tot["units_fail"] += int((~ok_unit).sum())
        # frontier of (ray, internal node) pairs, level by level
        ray = np.nonzero(ok_unit[unit] & np.all(d != 0, 1))[0]
        node = np.zeros(len(ray), np.int64)
        s_all = cc.signs(d)
        while len(ray):
            hm, _ = cc.expand(box[node, :3], box[node, 3:], o[ray], d[ray])
            hm &= wb[node]
            cnt = np.array([bin(i).count("1") for i in range(256)])[hm]
            chain = cc.CHAIN_VALID[s_all[ray], hm]
            key = unit[ray].astype(np.int64) * len(wa) + node  # one wave expansion
            uk, inv = np.unique(key, return_inverse=True)
            orders = np.zeros(len(uk), bool)
            bad = np.zeros(len(uk), bool)
            np.logical_or.at(orders, inv, cnt >= 2)
            np.logical_or.at(bad, inv, ~chain)
            tot["exp"] += len(uk)
            tot["exp_order"] += int(orders.sum())
            tot["exp_nonchain"] += int((orders & bad).sum())
            nr, nn = [], []
            for ci in range(8):
                take = ((hm >> np.uint32(ci)) & 1).astype(bool)
                child = wa[node[take]].astype(np.int64) + ci
                inner = (wa[child] & LEAF) == 0
                nr.append(ray[take][inner])
                nn.append(child[inner])
            ray, node = np.concatenate(nr), np.concatenate(nn)
    tot["units_fail_fraction"] = round(tot["units_fail"] / tot["units"], 5)
    tot["nonchain_fraction_of_ordering_expansions"] = round(tot["exp_nonchain"] / max(1, tot["exp_order"]), 5)
    tot["ord_wmin"] = [float(x) for x in wmin]
    print(json.dumps(tot))


if __name__ == "__main__":
    main()
