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
    kind = np.zeros(len(prims["type"]), np.int32)
    members_short, members_tall = _cornell_block_members(prims)
    kind[members_short] = short
    kind[members_tall] = tall
    return kind


def _cornell_block_members(prims):
    """the primitive indices of the Cornell box's short and tall block (cornell_blocks says how they are found)"""
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
    return blocks[0][1], blocks[1][1]


def _corners(types, verts):
    """per primitive the (3 or 4, 3) float32 corners that are read, with -0.0 and 0.0 made one"""
    verts = np.asarray(verts, np.float32) + np.float32(0.0)
    return [verts[i, :4 if types[i] == 1 else 3] for i in range(len(types))]


def icosphere(center, radius, level):
    """A sphere of 20 * 4**level triangles: the icosahedron, each triangle cut into four `level` times, every vertex pushed onto
    the sphere.  Returns (types (n,), verts (n, 4, 3), normal (n, 3), corner_normals (n, 4, 3)), float32, in the layout of
    ptmi_load_scene_arrays and Renderer.set_vertex_normals.  A vertex is computed once, so shared corners are bit-equal; the
    stored normal is the outward geometric one; a corner's normal is unit(corner - center)."""
    c = np.asarray(center, np.float64)
    t = (1.0 + np.sqrt(5.0)) / 2.0
    pts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    pts = [np.asarray(p, np.float64) / np.sqrt(1.0 + t * t) for p in pts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = pts[a] + pts[b]
                pts.append(m / np.linalg.norm(m))
                mid[key] = len(pts) - 1
            return mid[key]
        cut = []
        for a, b, d in faces:
            ab, bd, da = midpoint(a, b), midpoint(b, d), midpoint(d, a)
            cut += [(a, ab, da), (b, bd, ab), (d, da, bd), (ab, bd, da)]
        faces = cut
    unit = np.asarray(pts)
    pos = (c + float(radius) * unit).astype(np.float32)                # one float32 position per vertex: shared corners are bit-equal
    out = pos.astype(np.float64) - c
    vn = (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)
    idx = np.asarray(faces)
    n = len(idx)
    verts = np.zeros((n, 4, 3), np.float32); corner_normals = np.zeros((n, 4, 3), np.float32)
    verts[:, :3] = pos[idx]; corner_normals[:, :3] = vn[idx]
    v = verts.astype(np.float64)
    g = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert (np.einsum("ij,ij->i", g, v[:, 0] - c) > 0).all()             # counter-clockwise seen from outside
    return np.zeros(n, np.int32), verts, g.astype(np.float32), corner_normals


def smooth_normals(prims, crease_deg=40.0, flat_deg=1.0):
    """Corner normals for Renderer.set_vertex_normals from the stored normals of any loaded scene: (n_prims, 4, 3) float32.
    prims: dict(type, verts, normal, ...) (Renderer.scene_prims(), HostScene.prims()).  Corners are joined where their float32
    coordinates are EQUAL, as cornell_blocks joins them.  A corner's normal is the unit sum of the unit stored normals of the
    primitives around it - this one included - that lie within crease_deg of this primitive's, each weighted by the angle its
    primitive has at the corner.  Where every one of them lies within flat_deg of this primitive's stored normal (a planar
    neighbourhood, a corner nobody shares) or the sum has no direction, the corner keeps the stored normal bit for bit, so a
    scene of planes such as cbox.obj gives an all-flat table.  flat_deg is 1 degree and not 0 because modelled planes are not
    exact - the two triangles of cbox.obj's left wall differ by 0.47 degrees - while a curved mesh whose neighbouring facets
    differ by less than that (a sphere of over 100 000 triangles) shows no facets that interpolation could remove."""
    types = np.asarray(prims["type"]); stored = np.asarray(prims["normal"], np.float32)
    corners = _corners(types, prims["verts"])
    n = len(types)
    with np.errstate(all="ignore"):
        un = stored.astype(np.float64) / np.linalg.norm(stored.astype(np.float64), axis=1, keepdims=True)
    around = {}                                                          # corner -> [(primitive, angle at the corner)]
    for i in range(n):
        v = corners[i].astype(np.float64); m = len(v)
        for k in range(m):
            a, b = v[(k + 1) % m] - v[k], v[(k - 1) % m] - v[k]
            la, lb = np.linalg.norm(a), np.linalg.norm(b)
            ang = np.arccos(np.clip(np.dot(a, b) / (la * lb), -1.0, 1.0)) if la > 0 and lb > 0 else 0.0
            around.setdefault(corners[i][k].tobytes(), []).append((i, ang))
    cos_crease = np.cos(np.radians(min(max(float(crease_deg), 0.0), 180.0)))
    cos_flat = np.cos(np.radians(float(flat_deg)))
    out = np.repeat(stored[:, None, :], 4, axis=1).copy()
    for i in range(n):
        if not np.isfinite(un[i]).all():
            continue
        for k in range(len(corners[i])):
            total = np.zeros(3); planar = True
            for j, ang in around[corners[i][k].tobytes()]:
                if np.isfinite(un[j]).all() and np.dot(un[i], un[j]) >= cos_crease - 1e-12:
                    total += ang * un[j]
                    planar = planar and (j == i or np.dot(un[i], un[j]) >= cos_flat)
            length = np.linalg.norm(total)
            if not planar and length > 0:
                out[i, k] = (total / length).astype(np.float32)
    return out


def cornell_spheres(prims, level=3):
    """The Cornell box with each block replaced by a sphere (icosphere of `level`) that stands on the floor over the block's
    footprint: the centre over the middle of the footprint's extent in x and z, the radius half the smaller of the two, the
    block's colour.  prims as for cornell_blocks (subdivided or not, triangles or quads).  Returns (arrays, corner_normals, ranges):
    arrays = (types, verts, normal, bsdf, Le) for Renderer.load_scene_arrays - the scene without the blocks, then the short
    block's sphere, then the tall one's; corner_normals (n, 4, 3) for Renderer.set_vertex_normals, the stored normal at every
    corner outside the spheres; ranges = dict(short=(first, end), tall=(first, end)), the spheres' index ranges, for set_surfaces."""
    F = np.float32
    types = np.asarray(prims["type"], np.int32)
    corners = _corners(types, prims["verts"])
    blocks = _cornell_block_members(prims)
    keep = np.ones(len(types), bool)
    for members in blocks:
        keep[members] = False
    parts = [[types[keep]], [np.asarray(prims["verts"], F)[keep]], [np.asarray(prims["normal"], F)[keep]], [np.asarray(prims["bsdf"], F)[keep]],
             [np.asarray(prims["Le"], F)[keep]]]
    table = [np.repeat(parts[2][0][:, None, :], 4, axis=1)]
    ranges, first = {}, int(keep.sum())
    for name, members in zip(("short", "tall"), blocks):
        v = np.concatenate([corners[i] for i in members]).astype(np.float64)
        lo, hi = v.min(0), v.max(0)
        r = 0.5 * min(hi[0] - lo[0], hi[2] - lo[2])
        st, sv, sn, sc = icosphere((0.5 * (lo[0] + hi[0]), lo[1] + r, 0.5 * (lo[2] + hi[2])), r, level)
        parts[0].append(st); parts[1].append(sv); parts[2].append(sn)
        parts[3].append(np.repeat(np.asarray(prims["bsdf"], F)[members[0]][None], len(st), 0)); parts[4].append(np.zeros((len(st), 3), F))
        table.append(sc)
        ranges[name] = (first, first + len(st)); first += len(st)
    arrays = tuple(np.concatenate(p) for p in parts)
    return arrays, np.concatenate(table).astype(F), ranges


def checker(n, a, b):
    """An (n, n, 3) float32 image of two colours: texel (j, i) is a where i + j is even and b where it is odd (linear RGB, as
    Renderer.set_albedo_texture takes it)."""
    n = int(n)
    if n < 1:
        raise ValueError("checker: n must be >= 1")
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    if a.shape != (3,) or b.shape != (3,):
        raise ValueError("checker: the colours must be (3,)")
    j, i = np.mgrid[0:n, 0:n]
    return np.where((((i + j) & 1) == 0)[:, :, None], a, b).astype(np.float32)


def box_uvs(prims, scale=1.0, origin=(0, 0, 0)):
    """(n_prims, 4, 2) float32 corner UVs for Renderer.set_albedo_texture: every primitive is projected onto the plane of its stored
    normal's dominant axis and uv = (the two remaining coordinates, in x, y, z order, - origin) / scale.  A corner's UV depends on
    its position and that axis only, so a wall of any tessellation gets one continuous map and coplanar primitives agree bit for
    bit at shared corners.  prims: Renderer.scene_prims() (type, verts, normal).  A triangle's 4th entry is zero."""
    types = np.asarray(prims["type"]); verts = np.asarray(prims["verts"], np.float32); normal = np.asarray(prims["normal"], np.float32)
    scale = np.float32(scale); origin = np.asarray(origin, np.float32)
    if not (np.isfinite(scale) and scale != 0):
        raise ValueError("box_uvs: scale must be a finite number other than 0")
    uv = np.zeros((len(types), 4, 2), np.float32)
    for i in range(len(types)):
        axis = int(np.argmax(np.abs(normal[i])))
        keep = [c for c in range(3) if c != axis]
        read = 4 if types[i] == 1 else 3
        uv[i, :read] = (verts[i, :read][:, keep] - origin[keep]) / scale
    return uv
