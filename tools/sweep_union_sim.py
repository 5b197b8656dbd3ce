#!/usr/bin/env python3
"""What a 64-lane wave of the sweep (csrc/traversal.h: intersect_sweep) pays per ray segment, simulated on the CPU.

The sweep walks the pre-order of the reference's tree once per wave: a node's slab test is issued if ANY lane's cursor stands on
it, a leaf's triangles are tested if any lane passed the leaf's box, and the second half of Moller-Trumbore is issued if any
lane passed the (a, u) tests of the first half.  So a wave pays for the UNION of its lanes' visits.  This script measures that
union on a frame like the benchmark's (c2: cbox.obj, depth 8) and asks what regrouping a workgroup's rays before the walk
could save.  No GPU: the tree and the primitives come from the CPU oracle (tests/oracle_binding.py: bvh(), prims()), the paths
from a numpy path tracer with the integrator's structure (emission, Russian roulette above depth 2, cosine sampling, the
depth limit, the next camera ray when a sample ends) and numpy's own random numbers - the figures are statistics, not frames.

  python tools/sweep_union_sim.py [--scene cbox.obj] [--width 1024] [--height 1024] [--rows 24] [--segments 40] [--first 12] [--depth 8]

The frame is width x height, of which --rows rows, evenly spaced, are traced (24 rows of 1024 pixels = 96 workgroups): a wave's
camera rays are then as close together as in the full frame.  Slots are pixels in row-major order, 256 to a workgroup, 64
consecutive ones to a wave (the kernels' default map).  Segments
--first .. --segments - 1 are counted: by then the lanes of a wave are spread over all depths, as in the body of a frame.

Reported, per wave-segment:
  the union of node visits, triangle first halves and second halves in today's slot order, with the lanes that take part;
  the estimated traversal instructions (31 per node pass, 31 per first half, 28 per second half - the kernel's ISA) when
  the 256 rays of a workgroup are sorted by a key before they are cut into waves, relative to today's order;
  how many second-half passes remain if a lane latches one pending second half and the wave flushes only when a lane needs
  a second latch or the leaf ends (closest_t must be final before the next slab test); if every lane keeps a list of its own and
  works it off at the leaf's end; if the wave keeps one queue across its lanes; and the bound, every leaf packed 64 to a pass;
  the slab-test passes of the leaf-only walk (SWEEP_LEAVES: one per leaf, whatever the rays do) against today's node passes
  (2 x the interior nodes the wave's union enters + 1), which is what decides whether a scene takes that walk.

--scene takes a file of the scenes directory or the name of a scene of tests/test_gpu_sweep_passes.py (tri64: its 64-triangle soup).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_binding import OracleScene, SCENES, camera_frame, default_camera  # noqa: E402

F = np.float32
WAVE, BLOCK = 64, 256
C_NODE, C_FIRST, C_SECOND = 31, 31, 28
T_MIN = F(1e-4)


def preorder(bvh):
    """the tree in the order the walks visit it: [(node, skip position)], skip = the position after the node's subtree"""
    order, skip = [], {}

    def visit(n):
        pos = len(order); order.append(n)
        if bvh["count"][n] == 0:
            visit(bvh["left"][n]); visit(bvh["right"][n])
        skip[pos] = len(order)
    visit(0)
    return order, skip


def triangles(prims):
    """every primitive as one or two triangles (a quad is (v00, v10, v11) and (v00, v11, v01)): (v0, e1, e2) per primitive"""
    out = []
    for t, v in zip(prims["type"], prims["verts"]):
        tri = [(v[0], v[1] - v[0], v[2] - v[0])]
        if t == 1:
            tri.append((v[0], v[2] - v[0], v[3] - v[0]))
        out.append(tri)
    return out


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def dot(a, b):
    return (a * b).sum(1)


class Walk:
    """one ray segment of N rays through the pre-order, recording who visited what"""

    def __init__(self, scene):
        self.bvh, self.prims = scene.bvh(), scene.prims()
        self.order, self.skip = preorder(self.bvh)
        self.tris = triangles(self.prims)
        # a column per triangle test, in walk order: (primitive, half)
        self.columns = [(int(p), h) for n in self.order if self.bvh["count"][n] > 0
                        for p in self.bvh["indices"][self.bvh["left"][n]:self.bvh["left"][n] + self.bvh["count"][n]] for h in range(len(self.tris[p]))]
        self.col_of = {c: i for i, c in enumerate(self.columns)}

    def run(self, o, d):
        n_rays = len(o)
        with np.errstate(divide="ignore"):
            inv = (F(1.0) / d).astype(F)
        closest = np.full(n_rays, np.finfo(F).max, F); hit = np.full(n_rays, -1, np.int32)
        cur = np.zeros(n_rays, np.int32)
        nodes = np.zeros((n_rays, len(self.order)), bool)                  # slab test issued for this lane
        first = np.zeros((n_rays, len(self.columns)), bool); second = np.zeros_like(first)
        leaf_cols = []
        for pos, n in enumerate(self.order):
            m = cur == pos
            if not m.any():
                continue
            nodes[m, pos] = True
            with np.errstate(invalid="ignore"):
                t0 = (self.bvh["bmin"][n] - o[m]) * inv[m]; t1 = (self.bvh["bmax"][n] - o[m]) * inv[m]
            lo = np.where(inv[m] < 0, t1, t0); hi = np.where(inv[m] < 0, t0, t1)
            tmin = np.fmax(np.fmax(lo[:, 0], T_MIN), np.fmax(lo[:, 1], lo[:, 2]))
            tmax = np.fmin(np.fmin(hi[:, 0], closest[m]), np.fmin(hi[:, 1], hi[:, 2]))
            passed = ~(tmax < tmin)
            idx = np.flatnonzero(m)
            cur[idx] = pos + 1
            if self.bvh["count"][n] == 0:
                cur[idx[~passed]] = self.skip[pos]
                continue
            at = idx[passed]
            cols = []
            for p in self.bvh["indices"][self.bvh["left"][n]:self.bvh["left"][n] + self.bvh["count"][n]]:
                for h, (v0, e1, e2) in enumerate(self.tris[p]):
                    c = self.col_of[(int(p), h)]; cols.append(c)
                    if not len(at):
                        continue
                    first[at, c] = True
                    oo, dd = o[at], d[at]
                    hh = cross(dd, np.broadcast_to(e2, dd.shape)); a = dot(np.broadcast_to(e1, dd.shape), hh)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        f = F(1.0) / a
                        s = oo - v0; u = f * dot(s, hh)
                        ok1 = (np.abs(a) >= F(1e-8)) & (u >= 0) & (u <= 1)
                        second[at, c] = ok1
                        q = cross(s, np.broadcast_to(e1, s.shape)); v = f * dot(dd, q); t = f * dot(np.broadcast_to(e2, q.shape), q)
                        acc = ok1 & (v >= 0) & (u + v <= 1) & (t >= T_MIN) & (t < closest[at])
                    closest[at[acc]] = t[acc]; hit[at[acc]] = p
            leaf_cols.append(cols)
        return hit, closest, nodes, first, second, leaf_cols


def cosine_sample(rng, n_vec):
    n = len(n_vec)
    u, v = rng.random(n, dtype=F), rng.random(n, dtype=F)
    r, phi = np.sqrt(u), F(2 * np.pi) * v
    x, y, z = r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(F(0), F(1) - u))
    a = F(1.0) / (F(1.0) + np.where(n_vec[:, 2] < F(-0.9999999), F(0), n_vec[:, 2]))
    b = -n_vec[:, 0] * n_vec[:, 1] * a
    tang = np.stack([F(1) - n_vec[:, 0] ** 2 * a, b, -n_vec[:, 0]], 1); bit = np.stack([b, F(1) - n_vec[:, 1] ** 2 * a, -n_vec[:, 1]], 1)
    down = n_vec[:, 2] < F(-0.9999999)
    tang[down] = (0, -1, 0); bit[down] = (-1, 0, 0)
    w = x[:, None] * tang + y[:, None] * bit + z[:, None] * n_vec
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(F)


def union_cost(sel, nodes, first, second):
    """sel: (waves, 64) lane indices -> per wave (node passes, first halves, second halves)"""
    return nodes[sel].any(1).sum(1), first[sel].any(1).sum(1), second[sel].any(1).sum(1)


def latched_passes(sel, second, leaf_cols):
    """second-half passes of each wave with a one-deep latch per lane: a pass when a lane needs a second latch, and at a leaf's end"""
    passes = np.zeros(len(sel), np.int64)
    for cols in leaf_cols:
        pending = np.zeros(sel.shape, bool)
        for c in cols:
            need = second[sel, c]
            conflict = (need & pending).any(1)
            passes += conflict
            pending[conflict] = False
            pending |= need
        passes += pending.any(1)
    return passes


def queue_passes(sel, second, leaf_cols, cap=64):
    """second-half passes of each wave with a per-wave queue across lanes: a leaf's (lane, triangle) second halves join the queue
    triangle by triangle; when it holds more than `cap` items it is worked off, 64 items to a pass, before the next triangle joins,
    and again at the leaf's end (closest_t must be final before the next slab test).  cap = 0 is today's pass per triangle."""
    passes = np.zeros(len(sel), np.int64)
    for cols in leaf_cols:
        q = np.zeros(len(sel), np.int64)
        for c in cols:
            full = q > cap
            passes += np.where(full, -(-q // WAVE), 0); q[full] = 0
            q += second[sel, c].sum(1)
        passes += -(-q // WAVE)
    return passes


def private_rounds(sel, second, leaf_cols):
    """second-half passes of each wave when every lane keeps its own pending second halves of the leaf and works them off at the
    leaf's end, one per round: the rounds of a leaf are the most any lane of the wave holds"""
    rounds = np.zeros(len(sel), np.int64)
    for cols in leaf_cols:
        rounds += second[sel][:, :, cols].sum(2).max(1)
    return rounds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cbox.obj"); ap.add_argument("--width", type=int, default=1024); ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--segments", type=int, default=40); ap.add_argument("--first", type=int, default=12)
    ap.add_argument("--depth", type=int, default=8); ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    n = a.width * a.rows
    assert n % BLOCK == 0, "width * rows must be a multiple of 256"
    if a.scene.endswith(".obj"):
        scene = OracleScene.load(os.path.join(SCENES, a.scene))
    else:
        sys.path.insert(0, os.path.join(ROOT, "cuda-pathtracer_amd", "python"))
        from test_gpu_sweep_passes import scene as test_scene
        scene = test_scene(a.scene)[1]
    walk = Walk(scene)
    P = walk.prims
    cf = camera_frame(default_camera(), a.width, a.height).as_array()
    org, llc, hor, ver = cf[0:3], cf[3:6], cf[6:9], cf[9:12]
    rng = np.random.default_rng(a.seed)
    rows = ((np.arange(a.rows) * 2 + 1) * a.height) // (2 * a.rows)
    px = (np.arange(n) % a.width).astype(F); py = rows[np.arange(n) // a.width].astype(F)

    def camera(idx):
        u = (px[idx] + rng.random(len(idx), dtype=F)) / F(a.width); v = (py[idx] + rng.random(len(idx), dtype=F)) / F(a.height)
        w = llc + u[:, None] * hor + v[:, None] * ver - org
        return np.broadcast_to(org, w.shape).copy(), (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(F)

    o, d = camera(np.arange(n))
    tp = np.ones((n, 3), F); depth = np.zeros(n, np.int32); origin_prim = np.full(n, -1, np.int32)
    today = np.arange(n).reshape(-1, WAVE)
    keys = ["direction octant", "major axis", "octant + origin primitive", "origin primitive", "camera / bounce", "identical node sets"]
    tot = {k: 0.0 for k in ["today"] + keys}
    acc = dict(nodes=0, first=0, second=0, latched=0, queued=0, private=0, packed=0, waves=0, lanes_node=0.0, lanes_first=0.0, lanes_second=0.0,
               ray_first=0, ray_second=0, rays=0, lanes_at_leaf=0.0, leaves=0)
    for seg in range(a.segments):
        hit, t, nodes, first, second, leaf_cols = walk.run(o, d)
        if seg >= a.first:
            un, uf, us = union_cost(today, nodes, first, second)
            acc["nodes"] += un.sum(); acc["first"] += uf.sum(); acc["second"] += us.sum(); acc["waves"] += len(today)
            acc["latched"] += latched_passes(today, second, leaf_cols).sum()
            acc["queued"] += queue_passes(today, second, leaf_cols).sum(); acc["private"] += private_rounds(today, second, leaf_cols).sum()
            acc["packed"] += sum(-(-second[today][:, :, cols].sum((1, 2)) // WAVE) for cols in leaf_cols).sum()
            acc["lanes_node"] += nodes.sum() / WAVE; acc["lanes_first"] += first.sum() / WAVE; acc["lanes_second"] += second.sum() / WAVE
            acc["ray_first"] += first.sum(); acc["ray_second"] += second.sum(); acc["rays"] += n
            for cols in leaf_cols:
                at = first[:, cols[0]][today].sum(1)
                acc["lanes_at_leaf"] += at[at > 0].sum(); acc["leaves"] += (at > 0).sum()
            tot["today"] += (C_NODE * un + C_FIRST * uf + C_SECOND * us).sum()
            octant = (d[:, 0] < 0) * 4 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 1
            major = np.abs(d).argmax(1) * 2 + (np.take_along_axis(d, np.abs(d).argmax(1)[:, None], 1)[:, 0] < 0)
            _, node_set = np.unique(nodes, axis=0, return_inverse=True)
            key_of = {"direction octant": octant, "major axis": major, "octant + origin primitive": octant * 1024 + origin_prim + 1,
                      "origin primitive": origin_prim, "camera / bounce": (depth > 0).astype(np.int64), "identical node sets": node_set.reshape(-1)}
            for k in keys:
                kk = np.asarray(key_of[k]).reshape(-1, BLOCK)
                sel = (np.argsort(kk, axis=1, kind="stable") + np.arange(0, n, BLOCK)[:, None]).reshape(-1, WAVE)
                un2, uf2, us2 = union_cost(sel, nodes, first, second)
                tot[k] += (C_NODE * un2 + C_FIRST * uf2 + C_SECOND * us2).sum()
        # shade: integrator()'s depth loop after the intersection
        end = hit < 0
        h = np.flatnonzero(~end)
        rr = h[depth[h] > 2]
        if len(rr):
            prob = np.minimum(tp[rr].max(1), F(0.95))
            kill = rng.random(len(rr), dtype=F) > prob
            tp[rr[~kill]] /= prob[~kill][:, None]
            end[rr[kill]] = True
        h = np.flatnonzero(~end)
        tp[h] *= P["bsdf"][hit[h]]
        end[h[np.linalg.norm(tp[h], axis=1) < 1e-5]] = True
        h = np.flatnonzero(~end)
        depth[h] += 1
        end[h[depth[h] >= a.depth]] = True
        h = np.flatnonzero(~end)
        nr = P["normal"][hit[h]]
        sn = np.where((dot(d[h], nr) < 0)[:, None], nr, -nr).astype(F)
        o[h] = o[h] + t[h][:, None] * d[h] + F(1e-4) * sn
        d[h] = cosine_sample(rng, sn)
        origin_prim[h] = hit[h]
        e = np.flatnonzero(end)
        o[e], d[e] = camera(e)
        tp[e] = 1; depth[e] = 0; origin_prim[e] = -1

    w = acc["waves"]
    n_nodes = len(walk.order); n_tri = len(walk.columns)
    print(f"{a.scene} {a.width}x{a.height}, {a.rows} rows = {n // BLOCK} workgroups, segments {a.first} - {a.segments - 1}, depth {a.depth}: "
          f"{n_nodes} nodes, {n_tri} triangle tests in the tree")
    print("| per wave-segment, today's slot order | passes | of | lanes busy |")
    print("|---|---|---|---|")
    for name, key, lanes, of in (("node slab tests", "nodes", "lanes_node", n_nodes), ("first halves", "first", "lanes_first", n_tri),
                                 ("second halves", "second", "lanes_second", n_tri)):
        print(f"| {name} | {acc[key] / w:.1f} | {of} | {acc[lanes] / max(acc[key], 1):.2f} |")
    print(f"a ray passes the (a, u) test for {acc['ray_second'] / acc['rays']:.1f} of its {acc['ray_first'] / acc['rays']:.1f} triangle tests; "
          f"{acc['lanes_at_leaf'] / max(acc['leaves'], 1):.1f} lanes at a leaf the wave enters")
    print(f"second-half passes with a one-deep latch and flush on conflict: {acc['latched'] / w:.1f} against {acc['second'] / w:.1f} today")
    print(f"lane-private pending lists, worked off at the leaf's end: {acc['private'] / w:.1f}; a per-wave queue across lanes, worked off above "
          f"{WAVE} items and at the leaf's end: {acc['queued'] / w:.1f}; every leaf's second halves packed {WAVE} to a pass: {acc['packed'] / w:.1f}")
    n_leaves = int((walk.bvh["count"] > 0).sum())
    print(f"slab-test passes per wave-segment: leaf-only walk {n_leaves} (the leaves), today {acc['nodes'] / w:.1f} "
          f"(the union enters {(acc['nodes'] / w - 1) / 2:.1f} of {n_nodes - n_leaves} interior nodes)")
    print("| regrouping key (256 rays sorted, then cut into waves) | relative traversal cost |")
    print("|---|---|")
    for k in keys:
        print(f"| {k} | {tot[k] / tot['today']:.3f} |")


if __name__ == "__main__":
    main()
