"""Procedural scenes for the stress configurations (BASELINE.json configs[4]).

tessellated_cornell(cells_u, cells_v): every quad of a quad-only scene (cbox_quads.obj) is cut into a
cells_u x cells_v grid, two triangles per cell, and every grid vertex is pushed along the quad's normal by
1e-3 * (hash32(vertex_id, seed) / 2^32 - 0.5) so that bounding boxes are not degenerate.  256 x 128 cells on the
16 quads give 1,048,576 triangles.  Materials are inherited; each triangle carries its geometric normal.
Returns arrays in the layout ptmi_load_scene_arrays / po_scene_from_arrays take.
"""
import numpy as np


def hash32(x, seed):
    """lowbias32-style integer hash, vectorised (uint32 in, uint32 out)."""
    x = (np.asarray(x, np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def tessellated_cornell(prims, cells_u=256, cells_v=128, seed=1, amplitude=1e-3):
    """prims: dict(type, verts, normal, bsdf, Le) of a quad-only scene (e.g. ptmi.HostScene.load(cbox_quads).prims())."""
    F = np.float32
    types, verts = prims["type"], prims["verts"].astype(F)
    assert (types == 1).all(), "expects a quad-only scene"
    nq = len(types)
    s = (np.arange(cells_u + 1, dtype=F) / F(cells_u))[None, :, None]      # along v00 -> v10
    t = (np.arange(cells_v + 1, dtype=F) / F(cells_v))[:, None, None]      # along v00 -> v01
    out_v, out_n, out_b, out_e = [], [], [], []
    for q in range(nq):
        v00, v10, v11, v01 = verts[q]
        # bilinear patch through the four corners
        P = ((F(1) - s) * (F(1) - t)) * v00 + (s * (F(1) - t)) * v10 + (s * t) * v11 + ((F(1) - s) * t) * v01
        n = np.cross(v10 - v00, v01 - v00).astype(np.float64); n = (n / np.linalg.norm(n)).astype(F)
        vid = (q * (cells_u + 1) * (cells_v + 1) + np.arange((cells_u + 1) * (cells_v + 1))).reshape(cells_v + 1, cells_u + 1)
        disp = (hash32(vid, seed).astype(np.float64) / 2.0 ** 32 - 0.5) * amplitude
        P = (P + disp[..., None].astype(F) * n).astype(F)
        p00, p10, p11, p01 = P[:-1, :-1], P[:-1, 1:], P[1:, 1:], P[1:, :-1]
        tri = np.stack([np.stack([p00, p10, p11], -2), np.stack([p00, p11, p01], -2)], 2).reshape(-1, 3, 3)
        out_v.append(tri)
        gn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
        gn /= np.maximum(np.linalg.norm(gn, axis=1, keepdims=True), 1e-30)
        out_n.append(gn.astype(F))
        out_b.append(np.repeat(prims["bsdf"][q][None], len(tri), 0)); out_e.append(np.repeat(prims["Le"][q][None], len(tri), 0))
    tri = np.concatenate(out_v)
    v4 = np.zeros((len(tri), 4, 3), F); v4[:, :3] = tri
    return dict(type=np.zeros(len(tri), np.int32), verts=v4, normal=np.concatenate(out_n).astype(F),
                bsdf=np.concatenate(out_b).astype(F), Le=np.concatenate(out_e).astype(F))


def sky(width, height, sun_dir=(0.35, 0.75, 0.55), sun_radiance=(400.0, 380.0, 340.0), sun_texels=1,
        zenith=(0.25, 0.45, 0.9), horizon=(0.8, 0.85, 0.9), ground=(0.12, 0.11, 0.1)):
    """A procedural environment map for Renderer.set_environment: (height, width, 3) float32, row 0 at +y.  Rows are the bands
    cos(pi r / height) .. cos(pi (r + 1) / height) of the direction's y, columns divide the angle from +x towards +z evenly
    (include/ptmi.h: "environment lighting").  The upper rows blend horizon -> zenith by the band centre's height, the lower rows
    are `ground`, and the texel that holds sun_dir (and its sun_texels - 1 right-hand neighbours) has sun_radiance ADDED: a
    small bright region that cosine sampling rarely finds and next-event estimation samples directly."""
    width, height = int(width), int(height)
    z = np.cos(np.pi * np.arange(height + 1) / height)
    mid = 0.5 * (z[:-1] + z[1:])
    t = np.clip(mid, 0.0, 1.0)[:, None]
    rows = np.where(mid[:, None] > 0, (1.0 - t) * np.asarray(horizon, np.float64) + t * np.asarray(zenith, np.float64),
                    np.asarray(ground, np.float64))
    env = np.repeat(rows[:, None, :], width, axis=1)
    d = np.asarray(sun_dir, np.float64)
    d = d / np.linalg.norm(d)
    r = int(np.clip(np.searchsorted(-z, -d[1], side="left") - 1, 0, height - 1))
    j = int(np.floor((np.arctan2(d[2], d[0]) / (2.0 * np.pi)) % 1.0 * width)) % width
    for k in range(max(int(sun_texels), 0)):
        env[r, (j + k) % width] += np.asarray(sun_radiance, np.float64)
    return env.astype(np.float32)


def cornell_blocks(prims, short=1, tall=2):
    """The kind array for Renderer.set_surfaces that makes the Cornell box's short block a mirror (1) and its tall block glass
    (2), or the kinds given as short and tall (3, rough metal, needs set_surfaces' roughness).  prims: dict(type, verts, normal, bsdf, Le) of the loaded scene (Renderer.scene_prims(), HostScene.prims()), subdivided
    or not, triangles or quads.  The blocks are found from the geometry: primitives that share a corner form a body; a block is
    a body that emits nothing and keeps clear of the scene's bounding box in x and z (walls, floor, ceiling and back wall reach
    it); the lower of the two is the short one."""
    types = np.asarray(prims["type"]); le = np.asarray(prims["Le"])
    # corners are joined where their float32 coordinates are EQUAL (+ 0.0 makes -0.0 and 0.0 one key): the loaders copy a shared
    # vertex bit for bit and subdivision takes the midpoint of the same two corners on both sides of an edge.  A scene whose
    # corners merely lie close together would fall apart into single primitives, and the call would say so (ValueError).
    verts = np.asarray(prims["verts"], np.float32) + np.float32(0.0)
    n = len(types)
    corners = [verts[i, :4 if types[i] == 1 else 3] for i in range(n)]
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    seen = {}
    for i in range(n):
        for c in corners[i]:
            j = seen.setdefault(c.tobytes(), i)
            parent[find(i)] = find(j)
    allv = np.concatenate(corners)
    lo, hi = allv.min(0), allv.max(0)
    margin = 1e-3 * (hi - lo)
    bodies = {}
    for i in range(n):
        bodies.setdefault(find(i), []).append(i)
    blocks = []
    for members in bodies.values():
        v = np.concatenate([corners[i] for i in members])
        inside = all((v[:, a] > lo[a] + margin[a]).all() and (v[:, a] < hi[a] - margin[a]).all() for a in (0, 2))
        if inside and not le[members].any():
            blocks.append((float(v[:, 1].max()), members))
    if len(blocks) != 2:
        raise ValueError(f"cornell_blocks: expected two blocks, found {len(blocks)} candidate bodies")
    blocks.sort(key=lambda b: b[0])
    kind = np.zeros(n, np.int32)
    kind[blocks[0][1]] = short
    kind[blocks[1][1]] = tall
    return kind
