#!/usr/bin/env python3
"""Command-line caller of the C ABI (SURVEY 8b lists a CLI among the callers; the reference itself has none, its
`main` ignores argv): load a scene, optionally run the radiosity pre-pass, render one frame, save a PNG.

  python tools/ptmi_render.py --scene tests/golden/scenes/cbox.obj --width 512 --height 512 --spp 64 --out cbox.png
  python tools/ptmi_render.py --scene ... --subdivision 2 --radiosity --sampling-mode 3 --out guided.png
  python tools/ptmi_render.py --scene ... --radiosity --integrator radiosity --out radiosity_view.png
  python tools/ptmi_render.py --scene ... --spp 8 --passes 16 --out progressive.png          (16 passes of 8 samples)
  python tools/ptmi_render.py --scene ... --spp 8 --adaptive 0.02 --counts-png counts.png   (passes until every pixel stops)
  python tools/ptmi_render.py --scene ... --spp 8 --denoise --out denoised.png             (a-trous denoiser, 5 iterations)
  python tools/ptmi_render.py --scene ... --spp 2 --adaptive --denoise --variance-guided --variance-png sd.png --out denoised.png
                              (the variance-guided filter, steered by the adaptive run's own per-pixel statistics)
  python tools/ptmi_render.py --scene ... --spp 8 --aov-png aov                              (aov_albedo/normal/depth.png)
  python tools/ptmi_render.py --scene ... --spp 4 --orbit 16 --yaw-step 2 --temporal --denoise --out-prefix orbit_
                               (16 views 2 degrees apart, each through the temporal accumulation and the denoiser)
  python tools/ptmi_render.py --scene ... --spp 4 --orbit 16 --temporal --denoise --variance-guided --variance-png sd.png --out last.png
                               (the history carries its luminance variance; the variance-guided filter over it is steered by that)
  python tools/ptmi_render.py --scene ... --sky --next-event --out sky.png                    (procedural sky with a sun)
  python tools/ptmi_render.py --scene ... --env map.npy --env-rotation 90 --out lit.png      ((h, w, 3) float radiance, row 0 up)
  python tools/ptmi_render.py --scene ... --mirror 12-21 --glass 22-31 --ior 1.5 --max-depth 8 --out blocks.png
                               (load-order primitive indices: cbox.obj's short block a mirror, its tall block glass)
  python tools/ptmi_render.py --scene ... --rough 22-31 --roughness 0.3 --next-event --max-depth 8 --out metal.png
                               (the tall block brushed metal: GGX, its Kd the tint)
  python tools/ptmi_render.py --scene ... --spheres --glass tall --rough short --next-event --max-depth 8 --out spheres.png
                               (the blocks replaced by smooth-shaded spheres: a glass ball and a brushed-metal one)
  python tools/ptmi_render.py --scene mesh.obj --smooth 40 --out smooth.png
                               (corner normals from the stored ones, joined across edges of less than 40 degrees)
  python tools/ptmi_render.py --scene ... --texture checker:8 --texture-prims 6-7 --texture-scale 2 --out floor.png
                               (an 8 x 8 checker on cbox.obj's floor, repeating every 2 scene units; --texture FILE.npy takes an
                                (h, w, 3) float image in LINEAR RGB - nothing is decoded from sRGB)
  python tools/ptmi_render.py --scene ... --texture checker:8 --texture-prims 6-7 --spp 8 --shaded-features --denoise --out floor.png
                               (the denoiser demodulates by the textured colour, so the checker stays sharp; with --smooth or
                                --spheres the feature normal is the interpolated one.  --shaded-features albedo | normal | both)
  python tools/ptmi_render.py --scene ... --aperture 0.3 --focus-at 400,300 --spp 64 --out dof.png
                               (a thin lens of radius 0.3 scene units, focused on what pixel (400, 300) shows - x from the left, y
                                from the bottom; --focus D names the distance along the optical axis instead; neither: the look-at point)
  python tools/ptmi_render.py --scene ... --fog 0.15 --fog-albedo 0.9,0.9,0.95 --fog-g 0.6 --next-event --spp 64 --out fog.png
                               (a homogeneous medium of extinction 0.15 per scene unit filling the scene's bounds, scattering
                                forward; --fog-box=x0,y0,z0,x1,y1,z1 names another box.  The denoisers' guides do not see the fog)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-pathtracer_amd", "python"))
import ptmi  # noqa: E402


def index_list(text, named=None):
    """'12-23,30' -> [12, ..., 23, 30]; ValueError names the item that is no index and no ascending range.  named: name ->
    (first, end) ranges an item may name instead (--spheres: short, tall)"""
    out = []
    for part in text.split(","):
        if named and part.strip() in named:
            out.extend(range(*named[part.strip()]))
            continue
        lo, dash, hi = part.strip().partition("-")
        if not lo.isdigit() or (dash and not hi.isdigit()) or (dash and int(hi) < int(lo)):
            raise ValueError(f"'{part.strip()}' is neither an index nor a range such as 12-23")
        out.extend(range(int(lo), int(hi if dash else lo) + 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--width", type=int, default=800); ap.add_argument("--height", type=int, default=800)   # DEFAULT_WIDTH/HEIGHT
    ap.add_argument("--spp", type=int, default=16); ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--seed-base", type=int, default=2023)
    ap.add_argument("--subdivision", type=int, default=0); ap.add_argument("--convert-quads", action="store_true")
    ap.add_argument("--sampling-mode", type=int, default=0, help="0 BSDF, 1/2/4 grid, 3 MIS (render_config.h:38-44)")
    ap.add_argument("--mis-bsdf-fraction", type=float, default=0.5)
    ap.add_argument("--integrator", choices=["path", "radiosity"], default="path")
    ap.add_argument("--radiosity", action="store_true", help="run the radiosity pre-pass first (needed by guided modes / the radiosity view)")
    ap.add_argument("--radiosity-steps", type=int, default=10); ap.add_argument("--mc-samples", type=int, default=64)
    ap.add_argument("--point-to-point", action="store_true")
    ap.add_argument("--filter", choices=["none", "bilateral", "gaussian"], default="none", help="Apply Filter & Rebuild CDFs")
    ap.add_argument("--yaw", type=float, default=None); ap.add_argument("--pitch", type=float, default=None); ap.add_argument("--fov", type=float, default=None)
    ap.add_argument("--passes", type=int, default=0, help="progressive: this many accumulation passes of --spp samples instead of one frame")
    ap.add_argument("--adaptive", type=float, nargs="?", const=-1.0, default=None, metavar="THRESHOLD",
                    help="adaptive: passes of --spp samples until every pixel has stopped (relative standard error THRESHOLD; "
                         "default: the library's); --passes then sets max_passes")
    ap.add_argument("--counts-png", default=None, help="with --passes / --adaptive: grey map of the samples per pixel (white = most)")
    ap.add_argument("--denoise", type=int, nargs="?", const=-1, default=None, metavar="ITERATIONS",
                    help="--out gets the image through the edge-avoiding a-trous denoiser (ITERATIONS, default 5)")
    ap.add_argument("--variance-guided", action="store_true", help="--denoise runs the variance-guided filter: steered by the "
                    "accumulation's per-pixel statistics after --adaptive / --passes, by the history's own luminance variance with "
                    "--orbit --temporal, by a spatial estimate after a frame")
    ap.add_argument("--variance-png", default=None, metavar="FILE", help="with --variance-guided: the standard deviation left after "
                    "the filter, sqrt(variance_out), through the tone map")
    ap.add_argument("--aov-png", default=None, metavar="PREFIX", help="write PREFIX_albedo.png, PREFIX_normal.png, PREFIX_depth.png "
                    "from the feature buffers of the denoiser")
    ap.add_argument("--shaded-features", nargs="?", const="both", default=None, choices=["albedo", "normal", "both"],
                    help="--denoise, --variance-guided, --temporal and --aov-png read feature buffers that hold the textured albedo "
                    "(--texture) and / or the interpolated normal (--smooth, --spheres); default both")
    ap.add_argument("--orbit", type=int, default=0, metavar="FRAMES", help="render FRAMES views, --yaw-step degrees apart, one frame each")
    ap.add_argument("--yaw-step", type=float, default=2.0, metavar="DEG")
    ap.add_argument("--temporal", action="store_true", help="with --orbit: every view through the temporal accumulation (reprojected history)")
    ap.add_argument("--out-prefix", default=None, help="with --orbit: write every view to PREFIXnnn.png")
    ap.add_argument("--next-event", action="store_true", help="next-event estimation with MIS: sample the emitters at every bounce")
    ap.add_argument("--env", default=None, metavar="FILE.npy", help="environment light: a (height, width, 3) float lat-long radiance map, row 0 at +y")
    ap.add_argument("--sky", action="store_true", help="environment light: the procedural sky of ptmi_scenes.sky (gradient + sun)")
    ap.add_argument("--env-scale", type=float, default=1.0); ap.add_argument("--env-rotation", type=float, default=0.0, metavar="DEG")
    ap.add_argument("--env-fraction", type=float, default=0.5, help="with --next-event: share of the light samples that go to the environment")
    ap.add_argument("--mirror", default=None, metavar="LIST", help="specular surfaces: load-order primitive indices and ranges, e.g. 12-23,30")
    ap.add_argument("--glass", default=None, metavar="LIST"); ap.add_argument("--ior", type=float, default=1.5, help="index of refraction of --glass")
    ap.add_argument("--rough", default=None, metavar="LIST", help="rough metal (GGX): primitive indices and ranges like --mirror")
    ap.add_argument("--roughness", type=float, default=0.3, help="roughness of --rough, in [0.05, 1]; alpha is its square")
    ap.add_argument("--smooth", type=float, nargs="?", const=40.0, default=None, metavar="DEG",
                    help="smooth shading: corner normals from the stored ones (ptmi_scenes.smooth_normals), creases above DEG (default 40) stay")
    ap.add_argument("--spheres", type=int, nargs="?", const=3, default=None, metavar="LEVEL",
                    help="the Cornell box's blocks replaced by smooth-shaded spheres of 20 * 4^LEVEL triangles (default 3); "
                         "--mirror / --glass / --rough may then name them: short, tall")
    ap.add_argument("--texture", default=None, metavar="FILE.npy|checker[:N]",
                    help="albedo texture: a (height, width, 3) float image in linear RGB (no sRGB decoding), row 0 at v = 0, or an N x N "
                         "checker (default 8) of white and 0.2 grey; Kd is multiplied by it, UVs from ptmi_scenes.box_uvs")
    ap.add_argument("--texture-prims", default=None, metavar="LIST", help="the textured primitives, like --mirror; default: all that emit nothing")
    ap.add_argument("--texture-scale", type=float, default=1.0, metavar="X", help="scene units per repeat of the image")
    ap.add_argument("--texture-filter", choices=["nearest", "bilinear"], default="bilinear")
    ap.add_argument("--aperture", type=float, default=0.0, metavar="R", help="thin lens: the lens radius in scene units (0: the pinhole)")
    ap.add_argument("--focus", type=float, default=None, metavar="D", help="with --aperture: the focus distance along the optical axis "
                    "(default: the distance to the look-at point)")
    ap.add_argument("--focus-at", default=None, metavar="X,Y", help="with --aperture: focus on what the pixel shows (x from the left, y from the bottom)")
    ap.add_argument("--fog", type=float, default=0.0, metavar="SIGMA", help="participating medium: the extinction per scene unit (0: none)")
    ap.add_argument("--fog-albedo", default="1,1,1", metavar="R,G,B", help="with --fog: the single-scattering albedo, each in [0, 1]")
    ap.add_argument("--fog-g", type=float, default=0.0, metavar="G", help="with --fog: the Henyey-Greenstein asymmetry, |G| <= 0.9, > 0 forward")
    ap.add_argument("--fog-box", default=None, metavar="x0,y0,z0,x1,y1,z1", help="with --fog: the medium's box (default: the scene's bounds, padded by a thousandth of their largest extent; write --fog-box=-1,0,... where it starts with a minus)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="PNG file (top row first, like the reference's Save PNG)")
    a = ap.parse_args()

    r = ptmi.Renderer(a.device)
    t = time.time()
    r.load_scene(a.scene, a.subdivision, a.convert_quads)
    corner_normals, spheres = None, None
    if a.spheres is not None:
        import ptmi_scenes
        try:
            arrays, corner_normals, spheres = ptmi_scenes.cornell_spheres(r.scene_prims(), a.spheres)
        except ValueError as e:
            ap.error(f"--spheres needs the Cornell box: {e}")
        r.load_scene_arrays(*arrays)
    info = r.scene_info()
    print(f"scene: {info['n_prims']} primitives ({info['n_tris']} triangles, {info['n_quads']} quads), "
          f"{info['n_bvh_nodes']} BVH nodes, depth {info['bvh_depth']}  [{time.time() - t:.2f} s]")
    if a.radiosity:
        st = r.run_radiosity_solver(num_iterations=a.radiosity_steps, mc_samples=a.mc_samples, use_monte_carlo=not a.point_to_point)
        print(f"radiosity: {st.pairs} pairs, {st.rays} shadow rays, form factors {st.form_factor_ms:.1f} ms, "
              f"iterations {st.iteration_ms:.1f} ms, grids {st.grid_ms:.1f} ms")
        if a.filter != "none":
            r.apply_grid_filter(a.filter == "bilateral")
    cam = ptmi.default_camera()
    if a.yaw is not None: cam.yaw_deg = a.yaw
    if a.pitch is not None: cam.pitch_deg = a.pitch
    if a.fov is not None: cam.vfov_deg = a.fov
    r.set_camera(cam)
    r.update_resolution(a.width, a.height)
    r.set_config(spp=a.spp, max_depth=a.max_depth, seed_base=a.seed_base, sampling_mode=a.sampling_mode,
                 mis_bsdf_fraction=a.mis_bsdf_fraction, integrator=1 if a.integrator == "radiosity" else 0, next_event=a.next_event)
    if a.env or a.sky:
        if a.env and a.sky:
            ap.error("--env and --sky exclude each other")
        if a.sky:
            import ptmi_scenes
            env = ptmi_scenes.sky(64, 32)
        else:
            import numpy as np
            env = np.load(a.env)
        r.set_environment(env, scale=a.env_scale, rotation_deg=a.env_rotation, select_fraction=a.env_fraction)
        ei = r.environment_info()
        print(f"environment: {ei['width']}x{ei['height']}, total power {ei['total']:.4g}")
    if a.mirror or a.glass or a.rough:
        import numpy as np
        kind = np.zeros(info["n_prims"], np.int32)
        for text, value in ((a.mirror, ptmi.SURFACE_MIRROR), (a.glass, ptmi.SURFACE_GLASS), (a.rough, ptmi.SURFACE_ROUGH)):
            try:
                idx = index_list(text, spheres) if text else []
            except ValueError as e:
                ap.error(f"--mirror / --glass / --rough: {e}")
            if idx and not (0 <= min(idx) and max(idx) < len(kind)):
                ap.error(f"--mirror / --glass / --rough: the scene has primitives 0 .. {len(kind) - 1}")
            kind[idx] = value
        r.set_surfaces(kind, a.ior, a.roughness if a.rough else None)
        si = r.surfaces_info()
        print(f"surfaces: {si['n_mirror']} mirror, {si['n_glass']} glass primitives, ior {a.ior}")
        if a.rough:
            print(f"surfaces: {r.surface_counts()[3]} rough-metal primitives, roughness {a.roughness}")
    if a.smooth is not None:
        import ptmi_scenes
        prims = r.scene_prims()
        table = ptmi_scenes.smooth_normals(prims, a.smooth)
        if corner_normals is not None:                         # the spheres keep their own
            first = min(lo for lo, _ in spheres.values())
            table[first:] = corner_normals[first:]
        corner_normals = table
    if corner_normals is not None:
        r.set_vertex_normals(corner_normals)
        print(f"vertex normals: {r.vertex_normals_info()['n_smooth']} smooth primitives")
    if a.texture:
        import numpy as np
        import ptmi_scenes
        if a.texture == "checker" or a.texture.startswith("checker:"):
            try:
                image = ptmi_scenes.checker(int(a.texture[8:]) if a.texture[7:] else 8, (1.0, 1.0, 1.0), (0.2, 0.2, 0.2))
            except ValueError as e:
                ap.error(f"--texture: {e}")
        else:
            image = np.load(a.texture)
        prims = r.scene_prims()
        textured = prims["Le"].max(1) <= 0
        if a.texture_prims:
            try:
                idx = index_list(a.texture_prims, spheres)
            except ValueError as e:
                ap.error(f"--texture-prims: {e}")
            if idx and not (0 <= min(idx) and max(idx) < len(textured)):
                ap.error(f"--texture-prims: the scene has primitives 0 .. {len(textured) - 1}")
            textured[:] = False
            textured[idx] = True
        if not (a.texture_scale > 0):
            ap.error("--texture-scale must be positive")
        r.set_albedo_texture(image, ptmi_scenes.box_uvs(prims, a.texture_scale), textured, a.texture_filter)
        ti = r.albedo_texture_info()
        print(f"albedo texture: {ti['width']} x {ti['height']}, {a.texture_filter}, {ti['n_textured']} textured primitives")
    if a.shaded_features:
        r.set_feature_shading(albedo=a.shaded_features in ("albedo", "both"), normal=a.shaded_features in ("normal", "both"))
        fs = r.feature_shading()
        print(f"shaded features: albedo {'on' if fs['albedo'] else 'off'}, normal {'on' if fs['normal'] else 'off'}")
    if a.focus is not None and a.focus_at is not None:
        ap.error("--focus and --focus-at exclude each other")
    if (a.focus is not None or a.focus_at is not None) and not a.aperture > 0:
        ap.error("--focus / --focus-at need --aperture R with R > 0")
    if a.aperture != 0:
        focus = a.focus
        if a.focus_at is not None:
            x, comma, y = a.focus_at.partition(",")
            if not (comma and x.strip().isdigit() and y.strip().isdigit()):
                ap.error("--focus-at takes a pixel as X,Y")
            try:
                focus = r.focus_distance_at(int(x), int(y))
            except ValueError as e:
                ap.error(f"--focus-at: {e}")
        try:
            r.set_lens(a.aperture, focus)
        except ptmi.PtmiError as e:
            ap.error(f"--aperture / --focus: {e}")
        print("lens: radius %g, focus distance %g" % r.lens())
    if a.fog != 0:
        try:
            albedo = [float(x) for x in a.fog_albedo.split(",")]
            box = None if a.fog_box is None else [float(x) for x in a.fog_box.split(",")]
        except ValueError:
            ap.error("--fog-albedo takes R,G,B and --fog-box x0,y0,z0,x1,y1,z1")
        if len(albedo) != 3 or (box is not None and len(box) != 6):
            ap.error("--fog-albedo takes R,G,B and --fog-box x0,y0,z0,x1,y1,z1")
        if box is None:                                # the scene's bounds, padded: a flat scene still has a box, and geometry
            b = r.scene_bvh()                          # on the bounds lies inside the medium and not on its face
            lo, hi = b["bmin"][0].astype(float), b["bmax"][0].astype(float)
            pad = 1e-3 * max(float((hi - lo).max()), 1e-3)
            box = [float(x) for x in lo - pad] + [float(x) for x in hi + pad]
        try:
            r.set_medium(box[:3], box[3:], a.fog, albedo, a.fog_g)
        except ptmi.PtmiError as e:
            ap.error(f"--fog: {e}")
        m = r.medium()
        print("fog: sigma_t %g, albedo (%g, %g, %g), g %g, box (%g, %g, %g) - (%g, %g, %g)" % ((m.sigma_t,) + tuple(m.albedo) + (m.g,) + tuple(m.lo) + tuple(m.hi)))
    if a.orbit > 0:
        if a.variance_png and not (a.variance_guided and a.denoise is not None):
            ap.error("--variance-png needs --denoise --variance-guided")
        orbit(r, a, cam)
        r.close()
        return
    if a.adaptive is not None or a.passes > 0:
        prm = {}
        if a.adaptive is not None:
            if a.adaptive >= 0: prm["threshold"] = a.adaptive
            if a.passes > 0: prm["max_passes"] = a.passes
            prm.setdefault("threshold", ptmi.default_adaptive_params().threshold)      # (no keywords would mean plain progressive)
            passes = r.render_adaptive(**prm)
        else:
            r.accum_reset()
            passes = [r.accum_pass(None) for _ in range(a.passes)]
        secs = sum(p.seconds for p in passes); samples = sum(p.samples for p in passes)
        print(f"{len(passes)} passes: {a.width}x{a.height}, {samples / (a.width * a.height):.2f} samples per pixel on average, "
              f"{secs * 1e3:.2f} ms = {samples / secs / 1e6:.1f} Msamples/s")
        if a.counts_png:
            counts = r.sample_counts().astype("float64")
            grey = (255.0 * counts / max(counts.max(), 1.0)).astype("uint8")
            ptmi.write_png(a.counts_png, grey[:, :, None].repeat(3, axis=2))
            print(f"wrote {a.counts_png}")
    else:
        st = r.render_frame()
        print(f"frame: {a.width}x{a.height} x {a.spp} spp in {st.seconds * 1e3:.2f} ms = {st.samples / st.seconds / 1e6:.1f} Msamples/s")
    if a.variance_png and not (a.variance_guided and a.denoise is not None):
        ap.error("--variance-png needs --denoise --variance-guided")
    if a.denoise is not None and a.variance_guided:
        prm = {} if a.denoise < 0 else {"iterations": a.denoise}
        rgb, _ = r.denoise_variance(**prm)
        ems, fms = r.variance_timing()
        print(f"denoise (variance-guided): features {r.denoise_timing()[0]:.3f} ms, variance estimate {ems:.3f} ms, filter {fms:.3f} ms")
        if a.variance_png:
            write_variance_png(r, a.variance_png)
    elif a.denoise is not None:
        prm = {} if a.denoise < 0 else {"iterations": a.denoise}
        rgb, _ = r.denoise(**prm)
        fms, dms = r.denoise_timing()
        print(f"denoise: features {fms:.3f} ms, filter {dms:.3f} ms")
    elif a.out:
        rgb, _ = r.read_image()
    if a.out:
        ptmi.write_png(a.out, rgb)
        print(f"wrote {a.out}")
    if a.aov_png:
        write_aovs(r, a.aov_png)
    r.close()


def orbit(r, a, cam):
    """--orbit: one frame per view, the camera turned by --yaw-step between views; each view optionally through the temporal
    accumulation (--temporal) and the denoiser (--denoise: over the history with --temporal, else over the frame)"""
    prm = {} if a.denoise is None or a.denoise < 0 else {"iterations": a.denoise}
    yaw0 = cam.yaw_deg
    guided_history = a.temporal and a.variance_guided and a.denoise is not None
    if guided_history:
        r.set_temporal_moments(1)                      # the history carries its luminance variance: it steers the filter over it
    for i in range(a.orbit):
        cam.yaw_deg = yaw0 + i * a.yaw_step
        r.set_camera(cam)
        st = r.render_frame()
        line = f"view {i}: yaw {cam.yaw_deg:.2f}, frame {st.seconds * 1e3:.2f} ms"
        if a.temporal:
            rgb, _, ts = r.temporal_accumulate()
            line += f", temporal {ts.seconds * 1e3:.3f} ms (accepted {ts.accepted}, rejected {ts.rejected}, missed {ts.missed})"
            if guided_history:
                rgb, _ = r.denoise_temporal_variance(**prm)
            elif a.denoise is not None:
                rgb, _ = r.denoise_temporal(**prm)
        elif a.denoise is not None:
            rgb, _ = r.denoise_variance(**prm) if a.variance_guided else r.denoise(**prm)
        else:
            rgb, _ = r.read_image()
        print(line)
        if a.out_prefix:
            ptmi.write_png(f"{a.out_prefix}{i:03d}.png", rgb)
    if a.out:
        ptmi.write_png(a.out, rgb)
        print(f"wrote {a.out}")
    if a.variance_png and a.orbit > 0:
        write_variance_png(r, a.variance_png)


def write_variance_png(r, path):
    """the standard deviation left after the last variance-guided filter, sqrt(variance_out), through the tone map"""
    import numpy as np
    sd = np.sqrt(r.variance()[1].astype(np.float64))
    grey = (255.99 * np.minimum((sd / (sd + 1.0)) ** (1.0 / 2.2), 1.0)).astype(np.uint8)
    ptmi.write_png(path, grey[:, :, None].repeat(3, axis=2))
    print(f"wrote {path}")


def write_aovs(r, prefix):
    """albedo as is, normal as 0.5 n + 0.5, depth (distance from the camera) as grey, near = white, misses black"""
    import numpy as np
    r.render_features(ptmi.default_denoise_params().feature_grid)
    f = r.features()
    to8 = lambda x: (255.99 * np.clip(x, 0.0, 1.0)).astype(np.uint8)
    ptmi.write_png(f"{prefix}_albedo.png", to8(f["albedo"]))
    ptmi.write_png(f"{prefix}_normal.png", to8(0.5 * f["normal"] + 0.5 * (f["hit_fraction"][..., None] > 0)))
    hit = f["hit_fraction"] > 0
    depth = np.linalg.norm(f["position"] - r.camera_frame()[:3], axis=2)
    near, far = (depth[hit].min(), depth[hit].max()) if hit.any() else (0.0, 1.0)
    grey = np.where(hit, 1.0 - (depth - near) / max(far - near, 1e-6), 0.0)
    ptmi.write_png(f"{prefix}_depth.png", to8(grey)[:, :, None].repeat(3, axis=2))
    print(f"wrote {prefix}_albedo.png, {prefix}_normal.png, {prefix}_depth.png")


if __name__ == "__main__":
    main()
