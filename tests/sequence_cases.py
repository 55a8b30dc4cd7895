"""Seeded call sequences: a context that has answered many calls (warm) must answer the next one as a fresh context does.

Three parts, none of them a test:

  the model      - the state that decides results and nothing else (Model), with the rules of include/rt_hip.h for what ends a running
                   image and what each call leaves alone, each cited where it is applied;
  the sequences  - TRIPLES, a table written by hand from the state groups of csrc/rt_internal.h (what warms a cache, what must end or
                   keep it, what uses it), and RANDOM, eight seeded walks over the operation classes that together contain every
                   ordered pair of classes;
  the runner     - run_sequence: every operation goes to the warm context and, through Model's recipe for it, to a fresh context that
                   uploads the scene as it stands, replays the running image's calls and runs the operation; everything compared is
                   compared by bytes.  There is no tolerance anywhere: the rest of the suite holds a fresh context to the oracle and to
                   the float64 statements, this holds the warm context to the fresh one.

Tree kind, light grids, beam lists, the refit's view, staging sizes, lanes and counters are deliberately NOT in the model: they must
never show.  A new cache in DeviceState / rt_ctx gets a row in TRIPLES ("Call sequences").

Pure numpy at import: the library and torch are touched by the runner only.
"""
import collections
import dataclasses
import functools

import numpy as np

from gpu_raytracer_amd import hostpack, scenes
from gpu_raytracer_amd import types as T

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------------------
# operations
# ---------------------------------------------------------------------------------------------------------------------------------
Op = collections.namedtuple("Op", "cls args")  # args: the sorted (name, value) pairs: hashable, printable, comparable


def op(cls, **kw):
    return Op(cls, tuple(sorted(kw.items())))


def arg(o):
    return dict(o.args)


CLASSES = (
    "upload", "update_host", "update_device", "update_spheres", "update_rebuild", "prepare_tree", "prepare_grids",
    "frame01", "frame2", "accumulate", "accumulate_restart", "adaptive", "batch", "aovs_denoise", "denoise", "reads", "dispatch",
    "rejected", "failed_upload",
)
SCENE_NAMES = ("cornell12", "soup1200", "soup1536", "empty")
SHAPES = ((64, 48), (37, 29), (96, 64))
VARIANTS = ("default", "kernel_sm", "kernel_v1", "kernel_pipeline", "no_beams", "no_shadow_grid")
BATCH_SIZES = (65, 130)  # one wave plus one, two waves plus two
# the eighteen calls that share run_batch's staging and the two volume pairs added since, plus the two ray generators
BATCH_KINDS = (
    "intersect", "occluded", "intersect_all", "surface", "ambient_occlusion", "direct_light", "radiance", "radiance_sh", "irradiance",
    "closest_point", "closest_point_all", "inside", "signed_distance", "overlap_box", "sweep_sphere", "sweep_box", "sweep_capsule",
    "contact_capsule", "overlap_obb", "sweep_obb", "camera_rays", "sample_rays",
)
REJECTED_KINDS = ("render_accumulate_mode0", "render_bounces", "adaptive_min_samples", "update_count", "prepare_bits", "query_flags",
                  "denoise_iterations", "aovs_mode")
READS = ("rgb32f", "combined", "channels", "hits")
MIN_SAMPLES = 4  # of every adaptive call (test_gpu_adaptive.MIN)


@functools.lru_cache(maxsize=None)
def base_scene(name):
    """Small enough for a fresh upload to cost milliseconds: the host tree and the one-pass kernel at 0 bounces (cornell12), the device
    build with spheres (soup1200), another light, sphere and material count for the pipeline's per-light state (soup1536), nothing."""
    if name == "cornell12":
        return scenes.cornell12()
    if name == "soup1200":
        return scenes.random_soup(1200, seed=5, size=0.4, n_spheres=3, n_lights=2)
    if name == "soup1536":
        return scenes.random_soup(1536, seed=6, n_spheres=0, n_lights=5, n_materials=6)
    if name == "empty":
        return scenes.empty_scene()
    raise KeyError(name)


def base_positions(name):
    return np.ascontiguousarray(base_scene(name).vertices["position"], dtype=F32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def positions(name, pos_key):
    """The positions `pos_key` names: None = as uploaded, else (kind, seed) - the motions of test_gpu_geometry_update._motion, always
    applied to the uploaded positions, so that a key names one array whatever came before."""
    p = base_positions(name).astype(np.float64)
    if pos_key is None or len(p) == 0:
        return np.ascontiguousarray(p.astype(F32)).reshape(-1, 3)
    kind, seed = pos_key
    rng = np.random.default_rng(seed)
    lo, hi = p.min(0), p.max(0)
    ext = float((hi - lo).max())
    if kind == "jitter":
        p = p + rng.normal(0.0, 0.003 * ext, p.shape)
    elif kind == "rigid":
        sub = np.arange(len(p)) < len(p) // 3
        a = 0.4 + 0.05 * seed
        rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c = p[sub].mean(0)
        p[sub] = (p[sub] - c) @ rot.T + c + np.array([0.05, 0.02, -0.03]) * ext
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(p.astype(F32))


@functools.lru_cache(maxsize=None)
def spheres(name, sph_key):
    """The spheres `sph_key` names: None = as uploaded, else a seed: centres, radii and materials moved from the uploaded ones."""
    s = base_scene(name).spheres.copy()
    if sph_key is None or len(s) == 0:
        return s
    rng = np.random.default_rng(1000 + sph_key)
    s["center"] += rng.normal(0.0, 0.2, s["center"].shape).astype(F32)
    s["radius"] *= F32(0.7 + 0.5 * rng.random())
    s["material_id"] = (s["material_id"] + 1 + sph_key) % len(base_scene(name).materials)
    return s


@functools.lru_cache(maxsize=None)
def scene_at(name, pos_key, sph_key):
    """The scene a fresh context uploads for the state (name, pos_key, sph_key): the fresh upload of the moved scene that
    test_gpu_geometry_update already trusts."""
    sc = base_scene(name)
    v = sc.vertices.copy()
    v["position"] = positions(name, pos_key)
    return dataclasses.replace(sc, vertices=v, spheres=spheres(name, sph_key))


def camera(name, cam):
    """Camera 0 is the scene's own; camera 1 stands a little to its right and above."""
    c = np.array(base_scene(name).camera, dtype=T.CAMERA).copy()
    if cam:
        c["position"] = c["position"] + np.array([0.3, 0.1, 0.0], F32)
    return c


def box_of(name):
    """The box query inputs are drawn from: that of the uploaded triangles, never the warm context's own answers."""
    p = base_positions(name)
    if len(p) == 0:
        return np.full(3, -1.0), np.full(3, 1.0)
    return p.min(0).astype(np.float64), p.max(0).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# constructors (the TRIPLES table and the random generator both go through them)
# ---------------------------------------------------------------------------------------------------------------------------------
def U(scene):
    return op("upload", scene=scene)


def UH(kind, seed):
    return op("update_host", kind=kind, seed=seed)


def UD(kind, seed):
    return op("update_device", kind=kind, seed=seed)


def US(seed):
    return op("update_spheres", seed=seed)


def UR(kind, seed, mem="host"):
    return op("update_rebuild", kind=kind, seed=seed, mem=mem)


def PT():
    return op("prepare_tree")


def PG():
    return op("prepare_grids")


def F01(mode=1, shape=(64, 48), cam=0, tile=0, bounces=4, counters=False):
    return op("frame01", mode=mode, shape=shape, cam=cam, tile=tile, bounces=bounces, counters=counters)


def _sampled(cls, shape, spp, bounces, seed, tile, share, cam, variant, wf_batch, wf_lanes, counters):
    assert shape in SHAPES and 1 <= spp <= 5 and 0 <= bounces <= 3 and tile in (0, 16, 32) and variant in VARIANTS
    assert wf_batch in (None, 1, 3) and wf_lanes in (None, 1, 2)
    return op(cls, shape=shape, spp=spp, bounces=bounces, seed=seed, tile=tile, share=share, cam=cam, variant=variant, wf_batch=wf_batch,
              wf_lanes=wf_lanes, counters=counters)


def F2(shape=(64, 48), spp=2, bounces=2, seed=3, tile=0, share=False, cam=0, variant="default", wf_batch=None, wf_lanes=None, counters=False):
    return _sampled("frame2", shape, spp, bounces, seed, tile, share, cam, variant, wf_batch, wf_lanes, counters)


def ACC(shape=(64, 48), spp=2, bounces=2, seed=3, tile=0, share=False, cam=0, variant="default", wf_batch=None, wf_lanes=None, counters=False, restart=False):
    return _sampled("accumulate_restart" if restart else "accumulate", shape, spp, bounces, seed, tile, share, cam, variant, wf_batch, wf_lanes, counters)


def AD(shape=(64, 48), spp=2, bounces=2, seed=3, tile=0, share=False, cam=0, variant="default", wf_batch=None, wf_lanes=None, counters=False):
    return _sampled("adaptive", shape, spp, bounces, seed, tile, share, cam, variant, wf_batch, wf_lanes, counters)


def B(kind, n=65, mem="host", counters=False, seed=11, k=2, samples=3):
    assert kind in BATCH_KINDS and mem in ("host", "device")
    return op("batch", kind=kind, n=n, mem=mem, counters=counters, seed=seed, k=k, samples=samples)


def AOVD(shape=(64, 48), spp=2, seed=3, cam=0, mem="host"):
    return op("aovs_denoise", shape=shape, spp=spp, seed=seed, cam=cam, mem=mem)


def DN(shape=(64, 48), seed=1, mem="host"):
    return op("denoise", shape=shape, seed=seed, mem=mem)


def RD(order=READS):
    assert sorted(order) == sorted(READS)
    return op("reads", order=tuple(order))


def DISP(shape=(64, 48), mode=1, tile=32, order_seed=0, read=True):
    return op("dispatch", shape=shape, mode=mode, tile=tile, order_seed=order_seed, read=read)


def REJ(kind):
    assert kind in REJECTED_KINDS
    return op("rejected", kind=kind)


def FAIL(scene, k=0):
    assert k in (0, 1, 2)
    return op("failed_upload", scene=scene, k=k)


def full_check():
    """What every sequence ends in: a mode-1 frame, a 2-spp extended frame and 256 fixed rays through rt_intersect."""
    return [F01(mode=1, shape=(64, 48)), F2(shape=(64, 48), spp=2, bounces=2, seed=3), B("intersect", n=256, seed=7)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def normalised(o):
    """The operation a fresh context runs for `o`: the same results by rt_hip.h, on the plainest path.  "The other RT_FLAG_* bits
    change no bits" (rt_hip.h:224, the RT_FLAG_KERNEL_* / NO_SHADOW_GRID / NO_BEAMS comments at :59-69: "same results"), the batch
    and lane knobs are sizing only (rt_frame.cpp), counters fill node_visits / tri_tests only (rt_hip.h:56, :336), and host and
    device memory hold the same bytes (rt_hip.h:306-309)."""
    a = arg(o)
    if o.cls in ("frame2", "accumulate", "accumulate_restart", "adaptive"):
        a.update(variant="default", wf_batch=None, wf_lanes=None, counters=False)
    elif o.cls == "frame01":
        a.update(counters=False)
    elif o.cls in ("batch", "aovs_denoise", "denoise"):
        a.update(mem="host")
        if o.cls == "batch":
            a.update(counters=False)
    elif o.cls == "update_rebuild":
        a.update(mem="host")
    elif o.cls == "dispatch":
        a.update(read=True)
    return op(o.cls, **a)


def image_key(o):
    """What an accumulating call must share with the previous one to continue its running image (rt_hip.h:222-224): camera, width,
    height, max_bounces, frame_seed, tile_size (0 read as RT_TILE_SIZE), tile_rank, tile_world and RT_FLAG_NO_SHADOWS (never set
    here); and whether it is adaptive (rt_hip.h:257-258: plain after adaptive starts a new image, and the reverse)."""
    a = arg(o)
    return (a["cam"], a["shape"], a["bounces"], a["seed"], a["tile"] or T.TILE_SIZE, 0, 2 if a["share"] else 1, o.cls == "adaptive")


Recipe = collections.namedtuple("Recipe", "scene pos sph history op")  # what a fresh context does to answer one step
Step = collections.namedtuple("Step", "code recipe samples check_tree")  # expected return code (None: the fresh context's), ...


class Model:
    """The state that decides results, and nothing else."""

    def __init__(self):
        self.scene = None      # the uploaded scene's name; None before an upload and after a failed one
        self.shapes = None     # the scene whose vertex and sphere counts the last successful upload set (what an update must match)
        self.pos = None        # positions key (positions())
        self.sph = None        # spheres key (spheres())
        self.image = None      # the running image: None or (image_key, [the accumulating calls since its restart])
        self.targets = None    # what the frame targets hold: None (rt_read_* answer RT_ERR_NOT_UPLOADED) or the Recipe that filled them
        self.since_upload = []

    def samples(self):
        return sum(arg(c)["spp"] for c in self.image[1]) if self.image else 0

    def legal(self, o):
        """An operation is legal once a scene has been uploaded, whatever the state; before the first upload only an upload is
        generated (the two ray generators, rt_denoise and rt_upload_textures need no scene by rt_hip.h:384, :1382, :1394, but no
        sequence uses that)."""
        return o.cls in ("upload", "failed_upload") or self.shapes is not None

    def recipe(self, o, history=()):
        return Recipe(self.scene, self.pos, self.sph, tuple(normalised(h) for h in history), normalised(o))

    def apply(self, o):
        """Advance by `o`; returns the Step the runner checks."""
        assert self.legal(o), o
        cls, a = o.cls, arg(o)
        self.since_upload.append(o)
        if cls == "upload":
            # rt_hip.h:225 the running image ends with rt_upload_scene*; rt_scene.cpp upload_common: the last frame goes with the scene
            self.scene = self.shapes = a["scene"]
            self.pos = self.sph = self.image = self.targets = None
            self.since_upload = [o]
            return Step(0, None, 0, True)
        if cls == "failed_upload":
            # rt_scene.cpp:269-271: "the context counts as nothing uploaded until EVERY device holds the whole new scene"
            self.scene = self.pos = self.sph = self.image = self.targets = None
            return Step(-2, None, 0, False)
        if self.scene is None:
            # rt_hip.h:45, :315 and every call's "a call before any upload is RT_ERR_NOT_UPLOADED"; what needs no scene answers as on a
            # context that never had one.  Nothing changes.
            return Step(None, self.recipe(o), 0, False)
        if cls == "rejected":
            # rt_hip.h:227 "A call rejected for its arguments changes nothing."
            return Step(-1, self.recipe(o), self.samples(), False)
        if cls in ("update_host", "update_device", "update_rebuild"):
            # rt_hip.h:225 the running image ends with rt_update_geometry; :1348 "rt_read_* still return the last frame"
            self.pos, self.image = (a["kind"], a["seed"]), None
            return Step(0, None, 0, True)
        if cls == "update_spheres":
            self.sph, self.image = a["seed"], None  # the same rule: any rt_update_geometry ends it
            return Step(0, None, 0, True)
        if cls in ("prepare_tree", "prepare_grids"):
            # rt_hip.h:226 the running image survives rt_prepare; :175-182 "same images": the last frame is left alone as well
            return Step(0, None, self.samples(), True)
        if cls in ("frame01", "frame2"):
            self.image = None  # rt_hip.h:225-226 "any rt_render without RT_FLAG_ACCUMULATE"
            self.targets = self.recipe(o)
            return Step(0, self.targets, 0, False)
        if cls in ("accumulate", "accumulate_restart", "adaptive"):
            key = image_key(o)
            if cls != "accumulate_restart" and self.image and self.image[0] == key:  # rt_hip.h:222-224, :257-259
                self.image[1].append(o)
            else:  # rt_hip.h:224 "otherwise the call starts a new one at sample 0 by itself, as RT_FLAG_ACCUMULATE_RESTART does"
                self.image = (key, [o])
            self.targets = self.recipe(o, self.image[1][:-1])
            return Step(0, self.targets, self.samples(), False)
        if cls == "dispatch":
            self.image = None  # rt_hip.h:225 the running image ends with rt_dispatch_tile
            self.targets = self.recipe(o)  # every tile and channel is dispatched: nothing of the texels before remains
            return Step(0, self.targets, 0, False)
        if cls == "reads":
            return Step(0 if self.targets else -4, self.targets, self.samples(), False)
        if cls in ("batch", "aovs_denoise", "denoise"):
            # rt_hip.h:227 the running image survives the queries, rt_aovs, rt_sample_rays, rt_denoise; :313, :1395 "leave the last frame alone"
            return Step(0, self.recipe(o), self.samples(), False)
        raise KeyError(cls)


def run_model(ops):
    """The Steps of a whole sequence (the CPU tests' view of it)."""
    m = Model()
    return [m.apply(o) for o in ops], m


# ---------------------------------------------------------------------------------------------------------------------------------
# TRIPLES: (what warms a cache, what must end or keep it, what uses it), one row per line of thought; GROUPS names the state group
# ---------------------------------------------------------------------------------------------------------------------------------
STATE_GROUPS = ("grids", "beams", "refit", "mirror", "pipeline", "targets", "sums", "staging", "denoiser", "counters", "pending", "errors")
PIPE = dict(variant="kernel_pipeline")
DL = dict(kind="direct_light")


def _row(group, *ops):
    assert group in STATE_GROUPS and 3 <= len(ops) <= 6, (group, len(ops))
    return group, list(ops)


TRIPLES = {
    # light grids and occluder map (DeviceState::Grids, Grids::tried): built by a frame or rt_prepare; ended by a host update, a device
    # update, a rebuild, the quality tree and an upload; kept by a spheres-only update; used by a pipeline frame, rt_direct_light with
    # the grids' bias (1e-3), an accumulating call and an adaptive call
    "grids_frame__host_update__pipeline_frame": _row("grids", U("soup1200"), F2(**PIPE), UH("jitter", 1), F2(**PIPE), B(**DL)),
    "grids_prepare__device_update__direct_light": _row("grids", U("soup1200"), PG(), UD("rigid", 2), B(**DL, n=130), F2(**PIPE)),
    "grids_frame__rebuild__accumulate": _row("grids", U("soup1536"), F2(), UR("rigid", 3), ACC(), ACC()),
    "grids_prepare__quality_tree__adaptive": _row("grids", U("soup1200"), PG(), PT(), AD(), AD(), AD()),
    "grids_frame__upload__pipeline_frame": _row("grids", U("soup1200"), F2(), U("soup1536"), F2(**PIPE), B(**DL)),
    "grids_prepare__spheres_update__pipeline_frame": _row("grids", U("soup1200"), PG(), US(1), F2(**PIPE), B(**DL)),
    "grids_direct_light_then_moved_box": _row("grids", U("soup1200"), PG(), B(**DL), UH("rigid", 5), PG(), B(**DL)),
    # beam lists (WfBuffers::beam_*): built per frame; across a change of camera, resolution, tile size or share, upload and update
    "beams_camera__resolution__tile__share": _row("beams", U("soup1200"), F2(**PIPE), F2(cam=1, **PIPE), F2(shape=(37, 29), **PIPE), F2(tile=16, **PIPE),
                                                   F2(tile=32, share=True, **PIPE)),
    "beams_update__upload": _row("beams", U("soup1200"), F2(**PIPE), UH("rigid", 4), F2(**PIPE), U("cornell12"), F2(**PIPE)),
    "beams_off_then_on": _row("beams", U("soup1536"), F2(variant="no_beams"), F2(**PIPE), UD("jitter", 2), F2(**PIPE)),
    # the refit's view (rt_ctx::rf_ready, DeviceState::Refit): made by the first update of a tree, gone with the tree
    "refit_update__quality_tree__update": _row("refit", U("soup1200"), UH("jitter", 1), PT(), UH("rigid", 2)),
    "refit_update__rebuild__update": _row("refit", U("soup1200"), UH("jitter", 1), UR("rigid", 2), UH("jitter", 3)),
    "refit_update__upload_other_scene__update": _row("refit", U("soup1200"), UH("jitter", 1), U("soup1536"), UH("rigid", 2)),
    "refit_host_tree__update__upload__update": _row("refit", U("cornell12"), UH("jitter", 1), U("soup1200"), UD("jitter", 2), US(2)),
    # the stale host mirror (host_geometry_stale, box_lo / box_hi, build_tris): a device-resident update, then each reader of the mirror
    "mirror_device_update__quality_tree": _row("mirror", U("soup1200"), UD("rigid", 1), PT(), F2(**PIPE)),
    "mirror_device_update__prepare_grids": _row("mirror", U("soup1200"), UD("rigid", 1), PG(), F2(**PIPE), B(**DL)),
    "mirror_device_update__first_extended_frame": _row("mirror", U("soup1200"), UD("rigid", 1), F2(**PIPE), B(**DL)),
    "mirror_device_update__rebuild": _row("mirror", U("soup1200"), UD("rigid", 1), UR("jitter", 2, mem="device"), PT()),
    "mirror_device_update__host_update": _row("mirror", U("soup1200"), UD("rigid", 1), UH("jitter", 2), PG(), F2(**PIPE)),
    "mirror_device_update__spheres__quality_tree": _row("mirror", U("soup1200"), UD("jitter", 3), US(3), PT(), PG()),
    # the pipeline allocation (DeviceState::Lanes, wf_spp, used_two_lanes): one shape, light count, spp and lane count at a time
    "pipeline_same_shape__upload_more_lights": _row("pipeline", U("soup1200"), F2(**PIPE), U("soup1536"), F2(**PIPE), U("soup1200"), F2(**PIPE)),
    "pipeline_another_spp": _row("pipeline", U("soup1536"), F2(spp=4, **PIPE), F2(spp=2, **PIPE), F2(spp=5, **PIPE)),
    "pipeline_lanes_2_1_2": _row("pipeline", U("soup1200"), F2(spp=4, wf_lanes=2, **PIPE), F2(spp=4, wf_lanes=1, **PIPE), F2(spp=4, wf_lanes=2, **PIPE)),
    "pipeline_batch_3_then_unset": _row("pipeline", U("soup1200"), F2(spp=5, wf_batch=3, **PIPE), F2(spp=5, **PIPE), F2(spp=5, wf_batch=1, wf_lanes=2, **PIPE)),
    # the frame targets (DeviceState::Targets): one resolution at a time, zeroed when made
    "targets_sizes": _row("targets", U("cornell12"), F01(shape=(96, 64)), F01(shape=(37, 29), mode=0), RD(), F2(shape=(96, 64), tile=32, share=True),
                          RD(("hits", "channels", "rgb32f", "combined"))),
    "targets_dispatch": _row("targets", U("cornell12"), F2(), DISP(read=True), F2(shape=(37, 29)), DISP(shape=(37, 29), mode=0, tile=16, read=False),
                             RD(("combined", "hits", "channels", "rgb32f"))),
    # the running sums and the adaptive selection (DeviceState::Accum, Adaptive::cap): a resolution or tile size that needs more blocks
    "sums_resolution": _row("sums", U("soup1200"), ACC(shape=(37, 29)), ACC(shape=(96, 64)), ACC(shape=(96, 64)), ACC(shape=(37, 29))),
    "sums_adaptive_cap_grows": _row("sums", U("soup1200"), AD(tile=16), AD(tile=16), AD(tile=32), AD(tile=0), AD(tile=0)),
    "sums_adaptive_stops_pixels": _row("sums", U("soup1200"), AD(), AD(), AD(), AD(spp=3), RD()),
    "sums_key_seed": _row("sums", U("soup1200"), ACC(), ACC(seed=4), ACC(seed=4), ACC(), ACC()),
    "sums_key_bounces_tile_share": _row("sums", U("soup1200"), ACC(), ACC(bounces=1), ACC(bounces=1, tile=32), ACC(bounces=1, tile=32, share=True),
                                        ACC(bounces=1, tile=32, share=True)),
    "sums_key_camera_shape": _row("sums", U("soup1200"), AD(), AD(cam=1), AD(cam=1), AD(cam=1, shape=(37, 29)), AD(cam=1, shape=(37, 29))),
    "sums_plain_then_adaptive_then_plain": _row("sums", U("cornell12"), ACC(), AD(), AD(), ACC(), ACC(restart=True)),
    # the query staging that the batch calls share (DeviceState::Query: in, out, counts, ao, paths)
    "staging_130_then_65": _row("staging", U("soup1200"), B("intersect", n=130), B("intersect", n=65), B("surface", n=130), B("occluded", n=65)),
    "staging_counts": _row("staging", U("soup1200"), B("intersect_all", n=130, k=16), B("overlap_box", n=65, k=32), B("inside", n=130),
                           B("closest_point_all", n=65, k=16)),
    "staging_ao_counts_are_added_to": _row("staging", U("soup1200"), B("ambient_occlusion", n=130), B("ambient_occlusion", n=65),
                                           B("ambient_occlusion", n=65, mem="device")),
    "staging_paths": _row("staging", U("soup1200"), B("radiance", n=130), B("radiance_sh", n=65), B("irradiance", n=130), B("radiance", n=65, samples=1)),
    "staging_ray_generators": _row("staging", U("soup1200"), B("camera_rays", n=130, mem="device"), B("sample_rays", n=65), B("camera_rays", n=65, k=1),
                                   B("sample_rays", n=130, mem="device", counters=True), B("intersect", n=130, mem="device", counters=True)),
    # the denoiser's planes (DeviceState::Denoise): grown on demand, kept until rt_destroy
    "denoiser_96x64_then_37x29": _row("denoiser", U("cornell12"), DN(shape=(96, 64)), DN(shape=(37, 29)), F2(shape=(37, 29)), AOVD(shape=(37, 29)),
                                      AOVD(shape=(96, 64), mem="device")),
    # the device counters that frames and queries both zero and read (DeviceState::counters)
    "counters_frame__query__path_query__plain_frame": _row("counters", U("soup1200"), F2(counters=True, variant="kernel_sm"), B("intersect", counters=True),
                                                           B("radiance", counters=True), B(**DL, counters=True), F01()),
    # a rejected call and a failed upload between two of the above
    "errors_rejected_between_accumulating_calls": _row("errors", U("soup1200"), ACC(), REJ("render_bounces"), ACC(), REJ("adaptive_min_samples"), ACC()),
    "errors_rejected_update_between_grids_and_frame": _row("errors", U("soup1200"), PG(), REJ("update_count"), F2(**PIPE), REJ("prepare_bits"), B(**DL)),
    "errors_failed_upload_between_grids_and_frame": _row("errors", U("soup1200"), PG(), FAIL("soup1536", 1), F2(), U("soup1200"), F2(**PIPE)),
    "errors_failed_upload_after_device_update": _row("errors", U("soup1200"), UD("rigid", 1), FAIL("soup1200", 2), UH("jitter", 1), U("soup1200"), PT()),
    "errors_rejected_query_between_staging_sizes": _row("errors", U("soup1200"), B("intersect_all", n=130, k=16), REJ("query_flags"), B("intersect_all", n=65),
                                                       REJ("denoise_iterations"), REJ("aovs_mode")),
}


def _class_example(cls, rng, m, turn=None):
    """One operation of class `cls` for model state `m`, drawn from `rng` (the random walks and the pending rows share it).  `turn`
    (the random walks'): the batch call, the rejected call and the kernel variant are taken in turn, so that each comes up."""
    pick = lambda seq: seq[int(rng.integers(len(seq)))]

    def in_turn(seq):
        if turn is None:
            return pick(seq)
        turn[seq] = turn.get(seq, -1) + 1
        return seq[turn[seq] % len(seq)]

    flip = lambda p=0.5: bool(rng.random() < p)
    if cls == "upload":
        return U(pick(SCENE_NAMES))
    if cls == "failed_upload":
        return FAIL(pick(SCENE_NAMES), int(rng.integers(3)))
    if cls in ("update_host", "update_device"):
        return op(cls, kind=pick(("jitter", "rigid")), seed=int(rng.integers(1, 6)))
    if cls == "update_rebuild":
        return UR(pick(("jitter", "rigid")), int(rng.integers(1, 6)), mem=pick(("host", "device")))
    if cls == "update_spheres":
        return US(int(rng.integers(1, 6)))
    if cls == "prepare_tree":
        return PT()
    if cls == "prepare_grids":
        return PG()
    if cls == "frame01":
        return F01(mode=int(rng.integers(2)), shape=pick(SHAPES), cam=int(rng.integers(2)), tile=pick((0, 16, 32)), counters=flip(0.25))
    if cls in ("frame2", "accumulate", "accumulate_restart", "adaptive"):
        if cls in ("accumulate", "adaptive") and m.image and m.image[0][7] == (cls == "adaptive") and flip(0.8):
            last = arg(m.image[1][-1])  # continue the running image: the key's fields as they are, the rest drawn anew
            kw = {k: last[k] for k in ("shape", "bounces", "seed", "tile", "share", "cam")}
        else:
            kw = dict(shape=pick(SHAPES), bounces=int(rng.integers(0, 4)), seed=int(rng.integers(1, 1000)), tile=pick((0, 16, 32)), share=flip(0.25),
                      cam=int(rng.integers(2)))
            if cls != "frame2" and m.image and flip():  # the running image's key but for ONE field: a new image all the same
                last = arg(m.image[1][-1])
                field = pick(("shape", "bounces", "seed", "tile", "share", "cam"))
                kw = dict({k: last[k] for k in kw}, **{field: kw[field]})
        kw.update(spp=2 if cls == "adaptive" else int(rng.integers(1, 6)), variant=in_turn(VARIANTS), wf_batch=pick((None, 1, 3)), wf_lanes=pick((None, 1, 2)),
                  counters=flip(0.25))
        return _sampled(cls, **kw)
    if cls == "batch":
        return B(in_turn(BATCH_KINDS), n=pick(BATCH_SIZES), mem=pick(("host", "device")), counters=flip(0.3), seed=int(rng.integers(1, 100)), k=pick((1, 2, 16)),
                 samples=int(rng.integers(1, 4)))
    if cls == "aovs_denoise":
        t = arg(m.targets.op) if m.targets and m.targets.op.cls in ("frame2", "accumulate", "accumulate_restart", "adaptive") else None
        if t:  # the AOVs of the last extended frame, and its image denoised
            return AOVD(shape=t["shape"], spp=max(2, min(m.samples() or t["spp"], 8)), seed=t["seed"], cam=t["cam"], mem=pick(("host", "device")))
        return AOVD(shape=pick(SHAPES), spp=int(rng.integers(1, 4)), seed=int(rng.integers(1, 1000)), mem=pick(("host", "device")))
    if cls == "denoise":
        return DN(shape=pick(SHAPES), seed=int(rng.integers(1, 100)), mem=pick(("host", "device")))
    if cls == "reads":
        return RD(tuple(READS[i] for i in rng.permutation(len(READS))))
    if cls == "dispatch":
        return DISP(shape=pick(SHAPES), mode=int(rng.integers(2)), tile=pick((16, 32, 128)), order_seed=int(rng.integers(100)), read=flip())
    if cls == "rejected":
        return REJ(in_turn(REJECTED_KINDS))
    raise KeyError(cls)


def _pending_rows():
    """A pending rt_dispatch_tile (rt_ctx::pending_dispatch) before each other operation class: whatever needs the result or an idle
    device waits for it first (rt_hip.h:24-28)."""
    rows = {}
    for i, cls in enumerate(CLASSES):
        rng = np.random.default_rng(500 + i)
        m = Model()
        head = [U("soup1200"), F2(), DISP(read=False, tile=16)]
        for o in head:
            m.apply(o)
        rows[f"pending_dispatch__{cls}"] = _row("pending", *head, _class_example(cls, rng, m))
    return rows


def _image_rows():
    """A running image across each operation class, plain and adaptive: what rt_hip.h:225-227 says ends it, ends it, and what it says
    the image survives leaves the next accumulating call continuing it."""
    rows = {}
    for i, cls in enumerate(CLASSES):
        for kind, make in (("plain", ACC), ("adaptive", AD)):
            rng = np.random.default_rng(700 + i)
            m = Model()
            head = [U("soup1200"), make(tile=32)] + ([make(tile=32)] if kind == "adaptive" else [])
            for o in head:
                m.apply(o)
            x = _sampled(cls, **dict(arg(head[1]), spp=2)) if cls in ("accumulate", "accumulate_restart", "adaptive") else _class_example(cls, rng, m)
            rows[f"image_{kind}_across__{cls}"] = _row("sums", *head, x, make(tile=32))
    return rows


TRIPLES.update(_pending_rows())
TRIPLES.update(_image_rows())


def triple(name):
    """The operations of a TRIPLES row, full check included."""
    ops = list(TRIPLES[name][1])
    m = run_model(ops)[1]
    return ops + ([] if m.scene else [U("soup1200")]) + full_check()


# ---------------------------------------------------------------------------------------------------------------------------------
# random sequences: eight committed seeds; together they contain every ordered pair of classes adjacent at least once
# ---------------------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = (101, 102, 103, 104, 105, 106, 107, 108)
RANDOM_LENGTH = 52          # operations per seed before the full check: about the least at which the eight cover every pair (test_sequence_cases.py)
MULTI_DEVICE_SEED = 104     # its warm context is api.Context((0, 0)); the reference stays on one device


def adjacent_pairs(ops):
    """The ordered pairs of classes a sequence contains.  A pair counts where its second operation meets an uploaded scene, or where
    its first is the failed upload (whose point is what the next call answers)."""
    m, out, prev = Model(), set(), None
    for o in ops:
        if prev is not None and (m.scene is not None or prev == "failed_upload"):
            out.add((prev, o.cls))
        m.apply(o)
        prev = o.cls
    return out


@functools.lru_cache(maxsize=None)
def random_sequences():
    """{seed: operations}.  The seeds are walked in the committed order and share the set of pairs already covered: each step prefers
    a class that closes an uncovered pair and leads to the most uncovered ones, ties broken by the seed's generator.  Deterministic."""
    covered, out, turn = set(), {}, {}
    for seed in RANDOM_SEEDS:
        rng = np.random.default_rng(seed)
        m = Model()
        ops = [U(SCENE_NAMES[1 + seed % 2])]
        m.apply(ops[0])
        while len(ops) < RANDOM_LENGTH:
            prev = ops[-1].cls
            if m.scene is None and prev != "failed_upload":
                cls = "upload"  # one call on the context without a scene is the point; then it gets one again
            else:
                todo = lambda c: sum((c, d) not in covered for d in CLASSES)
                fresh = [c for c in CLASSES if (prev, c) not in covered]
                pool = fresh or list(CLASSES)
                best = max(todo(c) for c in pool)
                pool = [c for c in pool if todo(c) == best]
                cls = pool[int(rng.integers(len(pool)))]
            o = _class_example(cls, rng, m, turn)
            if m.scene is not None or prev == "failed_upload":
                covered.add((prev, cls))
            m.apply(o)
            ops.append(o)
        if m.scene is None:
            ops.append(U("soup1200"))
        out[seed] = ops + full_check()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# query inputs: from the scene's box and a seed
# ---------------------------------------------------------------------------------------------------------------------------------
INPUT_OF = {
    "intersect": "rays", "occluded": "rays", "intersect_all": "rays", "surface": "rays", "radiance": "rays",
    "ambient_occlusion": "surface", "direct_light": "surface", "irradiance": "surface",
    "radiance_sh": "probes", "closest_point": "points", "closest_point_all": "points", "inside": "points", "signed_distance": "points",
    "overlap_box": "boxes", "overlap_obb": "obbs", "sweep_sphere": "sweeps", "sweep_box": "box_sweeps", "sweep_obb": "obb_sweeps",
    "sweep_capsule": "capsule_sweeps", "contact_capsule": "capsules",
}


@functools.lru_cache(maxsize=None)
def query_input(scene, kind, n, seed):
    """n records of `kind` for the scene named `scene`: float32, C-contiguous, read-only."""
    from gpu_raytracer_amd import api
    rng = np.random.default_rng([seed, n, sorted(set(INPUT_OF.values())).index(kind)])
    lo, hi = box_of(scene)
    ext = float((hi - lo).max()) + 1e-3
    inside = (lo + rng.random((n, 3)) * (hi - lo)).astype(F32)
    around = ((lo + hi) / 2 + rng.normal(0, 1, (n, 3)) * ext).astype(F32)
    dirs = rng.normal(0, 1, (n, 3))
    unit = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F32)
    half = (rng.random((n, 3)) * 0.1 * ext).astype(F32)
    quat = rng.normal(0, 1, (n, 4)).astype(F32)
    if kind == "rays":
        out = api.make_rays(around, inside - around, tmax=F32(3.0e38))
    elif kind == "surface":
        out = np.zeros((n, 8), F32)
        out[:, 0:3], out[:, 4:7] = inside, unit
        out.view(np.uint32)[:, 7] = rng.integers(0, max(1, len(base_scene(scene).materials)) + 1, n)  # one id past the table among them
        out[-1, 4:7] = 0.0  # what rt_surface writes for a miss: no point
    elif kind == "points":
        out = api.make_points(inside, (0.05 + 0.45 * rng.random(n)).astype(F32) * F32(ext))
    elif kind == "probes":
        out = api.make_probes(inside)
    elif kind == "sweeps":
        out = api.make_sweeps(around, inside - around, F32(0.03 * ext))
    elif kind == "boxes":
        out = api.make_boxes(inside, half)
    elif kind == "obbs":
        out = api.make_obbs(inside, half, quat)
    elif kind == "box_sweeps":
        out = api.make_box_sweeps(around, half, inside - around)
    elif kind == "obb_sweeps":
        out = api.make_obb_sweeps(around, half, quat, inside - around)
    elif kind == "capsules":
        out = api.make_capsules(inside, F32(0.08 * ext), (unit * F32(0.2 * ext)).astype(F32))
    elif kind == "capsule_sweeps":
        out = api.make_capsule_sweeps(around, (unit * F32(0.2 * ext)).astype(F32), inside - around, F32(0.03 * ext))
    else:
        raise KeyError(kind)
    out = np.ascontiguousarray(out, dtype=F32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def noise_image(shape, seed):
    """A random image and plausible feature records for rt_denoise alone: (rgb (h, w, 3), aov (h, w, 8))."""
    w, h = shape
    rng = np.random.default_rng([seed, w, h])
    rgb = rng.random((h, w, 3)).astype(F32)
    aov = np.zeros((h, w, 8), F32)
    aov[..., 0:3] = 0.2 + 0.6 * rng.random((h, w, 3))
    aov[..., 3] = 1.0 + 3.0 * rng.random((h, w))
    nrm = rng.normal(0, 1, (h, w, 3))
    aov[..., 4:7] = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
    aov[..., 7] = 1.0
    aov[h // 2:, : w // 3, 3:8] = 0.0  # a patch of misses
    for a in (rgb, aov):
        a.setflags(write=False)
    return rgb, aov


# ---------------------------------------------------------------------------------------------------------------------------------
# the runner (needs the library and a device)
# ---------------------------------------------------------------------------------------------------------------------------------
STAT_FIELDS = ("rays", "primary_rays", "continuation_rays", "shadow_rays", "pixels")  # not flags, node_visits, tri_tests, times


def np_error(rec):
    """rt_hip.h's adaptive error from (S, n, H) in numpy float32 and in its order (test_gpu_adaptive.np_error)."""
    s, n, hh = rec[..., 0:3], rec[..., 3], rec[..., 4:7]
    with np.errstate(all="ignore"):
        i = s / n[..., None]
        a = (hh + hh) / n[..., None]
        d = np.abs(i[..., 0] - a[..., 0]) + np.abs(i[..., 1] - a[..., 1]) + np.abs(i[..., 2] - a[..., 2])
        e = d / (F32(1e-4) + np.sqrt(i[..., 0] + i[..., 1] + i[..., 2]))
    return np.where(n == 0, F32(0), e).astype(F32)


def _bytes(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).tobytes()


def _to(mem, a):
    """The array in the kind of memory an operation draws: a writable host copy, or a tensor on the context's first device."""
    if mem == "host":
        return np.array(a, copy=True)
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def _frame_kw(scene, a, mode):
    kw = dict(mode=mode, frame_seed=a.get("seed", 0), tile_size=a["tile"], counters=a["counters"])
    if mode == 2:
        kw.update(spp=a["spp"], max_bounces=a["bounces"], tile_world=2 if a["share"] else 1)
        if a["variant"] != "default":
            kw[a["variant"]] = True
    else:
        kw.update(max_bounces=a["bounces"])
    return a["shape"][0], a["shape"][1], camera(scene, a["cam"]), kw


def _stats(ctx):
    st = ctx.stats()
    return {f"stats.{k}": st[k] for k in STAT_FIELDS}


def _read_all(ctx, hits):
    obs = {"rgb32f": _bytes(ctx.read_rgb32f()), "combined": _bytes(ctx.read_rgba8_combined())}
    obs["channels"] = b"".join(_bytes(c) for c in ctx.read_rgba8_channels())
    if hits:
        obs["hits"] = b"".join(_bytes(x) for x in ctx.read_hits())
    return obs


def _batch_call(api, ctx, scene, a):
    """One of the batch calls -> the tuple of its outputs."""
    kind, n, c = a["kind"], a["n"], a["counters"]
    if kind in ("camera_rays", "sample_rays"):
        w, h = 13, n // 13
        out = _to(a["mem"], np.zeros((w * h, 8), F32))
        if kind == "camera_rays":
            return (ctx.camera_rays(w, h, camera(scene, 0), mode=a["k"] % 2, out=out),)
        return (ctx.sample_rays(w, h, camera(scene, 0), a["samples"], out=out, spp=4, frame_seed=a["seed"]),)
    x = _to(a["mem"], query_input(scene, INPUT_OF[kind], n, a["seed"]))
    path = dict(samples=a["samples"], max_bounces=2, seed=a["seed"], counters=c)
    if kind in ("intersect", "occluded", "surface", "closest_point", "sweep_sphere", "sweep_box", "sweep_obb", "sweep_capsule"):
        return (getattr(ctx, kind)(x, counters=c),)
    if kind == "intersect_all":
        return ctx.intersect_all(x, min(a["k"], api.MULTI_HIT_MAX), count_all=a["k"] == 1, counters=c)
    if kind == "closest_point_all":
        return ctx.closest_point_all(x, min(a["k"], api.NEAREST_MAX), count_all=a["k"] == 1, counters=c)
    if kind in ("overlap_box", "overlap_obb"):
        return getattr(ctx, kind)(x, min(a["k"], api.OVERLAP_MAX), count_all=a["k"] == 1, counters=c)
    if kind == "contact_capsule":
        return ctx.contact_capsule(x, min(a["k"], api.CONTACT_MAX), count_all=a["k"] == 1, counters=c)
    if kind in ("inside", "signed_distance"):
        return getattr(ctx, kind)(x, rays=3, votes=True, counters=c)
    if kind == "ambient_occlusion":
        lo, hi = box_of(scene)
        return ctx.ambient_occlusion(x, a["samples"], seed=a["seed"], max_distance=float((hi - lo).max()), counters=c)
    if kind == "direct_light":
        return (ctx.direct_light(x, bias=1e-3, ambient=a["k"] == 16, counters=c),)  # the grids' bias: 1e-3f
    if kind == "radiance":
        return (ctx.radiance(x, **path),)
    if kind == "radiance_sh":
        return (ctx.radiance_sh(x, a["samples"], max_bounces=2, seed=a["seed"], counters=c),)
    if kind == "irradiance":
        return (ctx.irradiance(x, a["samples"], max_bounces=2, seed=a["seed"], counters=c),)
    raise KeyError(kind)


def _rejected(api, ctx, scene, kind):
    """One bad argument per family (the tables of test_accumulation_abi, test_gpu_adaptive, test_gpu_geometry_update,
    test_ray_query_abi, test_denoise_abi); raises the RtError."""
    import ctypes as C
    cam = camera(scene, 0)
    if kind == "render_accumulate_mode0":
        ctx.render(64, 48, cam, mode=0, accumulate=True)
    elif kind == "render_bounces":
        ctx.render(64, 48, cam, mode=2, spp=1, max_bounces=256)
    elif kind == "adaptive_min_samples":
        ctx.render_adaptive(64, 48, cam, 2, 0.1, min_samples=1)
    elif kind == "update_count":
        v = positions(scene, None)
        ctx._check(ctx.lib.rt_update_geometry(ctx._h, C.c_void_p(v.ctypes.data), C.c_uint32(len(v) + 1), None, C.c_uint32(0), C.c_uint32(0)))
    elif kind == "prepare_bits":
        ctx.prepare(0x80)
    elif kind == "query_flags":
        rays, hits = np.array(query_input(scene, "rays", 65, 1)), np.zeros((65, 4), F32)
        ctx._check(ctx.lib.rt_intersect(ctx._h, C.c_void_p(rays.ctypes.data), C.c_size_t(65), C.c_void_p(hits.ctypes.data), C.c_uint32(0x80)))
    elif kind == "denoise_iterations":
        rgb, aov = noise_image((37, 29), 1)
        ctx.denoise(np.array(rgb), np.array(aov), iterations=0)
    elif kind == "aovs_mode":
        ctx.aovs(64, 48, cam, mode=3)
    else:
        raise KeyError(kind)


def dispatch_jobs(a):
    """The (tile offset, tile size, channel) of a dispatch run: every tile of the frame and every channel, in a seeded order."""
    w, h = a["shape"]
    t = a["tile"]
    jobs = [((x, y), (min(t, w - x), min(t, h - y)), c) for y in range(0, h, t) for x in range(0, w, t) for c in range(3)]
    order = np.random.default_rng(a["order_seed"]).permutation(len(jobs))
    return [jobs[i] for i in order]


class Runner:
    """Runs operations on contexts and keeps what fresh contexts answered (one reference per recipe, shared by every test of the run)."""

    def __init__(self, api):
        self.api = api
        self.memo = {}        # Recipe -> observations of a fresh context
        self.thresholds = {}  # (scene, pos, sph, image key) -> adaptive threshold

    # -- one operation on one context -------------------------------------------------------------------------------------------
    def execute(self, ctx, o, scene, rgb_in=None, threshold=None, env=None, pending_ok=False):
        """Run `o` on `ctx` (scene: the name whose arrays the operation's inputs come from) -> {what: bytes or number}; "code" is the
        return code of the first call that failed, 0 otherwise."""
        api, a, cls, obs = self.api, arg(o), o.cls, {"code": 0}
        try:
            if cls in ("upload", "failed_upload"):
                if cls == "failed_upload":
                    import ctypes as C
                    assert ctx.lib.rt_debug_fail_upload(ctx._h, C.c_int(a["k"])) == 0
                ctx.upload_scene(base_scene(a["scene"]))
            elif cls in ("update_host", "update_device", "update_rebuild"):
                mem = "device" if cls == "update_device" else a.get("mem", "host")
                ctx.update_geometry(_to(mem, positions(scene, (a["kind"], a["seed"]))), rebuild=cls == "update_rebuild")
                obs.update(_stats(ctx))
            elif cls == "update_spheres":
                ctx.update_geometry(spheres=spheres(scene, a["seed"]).copy())
                obs.update(_stats(ctx))
            elif cls == "prepare_tree":
                ctx.prepare(api.PREPARE_QUALITY_TREE)
            elif cls == "prepare_grids":
                ctx.prepare(api.PREPARE_SHADOW_GRIDS)
            elif cls == "frame01":
                w, h, cam, kw = _frame_kw(scene, a, a["mode"])
                ctx.render(w, h, cam, **kw)
                obs.update(_stats(ctx))
                obs.update(_read_all(ctx, hits=True))
            elif cls in ("frame2", "accumulate", "accumulate_restart", "adaptive"):
                w, h, cam, kw = _frame_kw(scene, a, 2)
                for name, v in (("RT_WF_BATCH", a["wf_batch"]), ("RT_WF_LANES", a["wf_lanes"])):  # rt_frame.cpp reads both per frame
                    if env is not None and v is not None:
                        env.setenv(name, str(v))
                try:
                    if cls == "adaptive":
                        spp = kw.pop("spp")
                        ctx.render_adaptive(w, h, cam, spp, threshold, min_samples=MIN_SAMPLES, **kw)
                    else:
                        ctx.render(w, h, cam, accumulate=cls != "frame2", restart=cls == "accumulate_restart", **kw)
                finally:
                    if env is not None:
                        env.delenv("RT_WF_BATCH", raising=False)
                        env.delenv("RT_WF_LANES", raising=False)
                obs.update(_stats(ctx))
                obs.update(_read_all(ctx, hits=False))
                if cls == "adaptive":
                    obs["adaptive"] = _bytes(ctx.read_adaptive())
            elif cls == "batch":
                for i, out in enumerate(_batch_call(api, ctx, scene, a)):
                    obs[f"out{i}"] = _bytes(out)
                if a["kind"] not in ("camera_rays", "sample_rays"):  # rt_hip.h:1383 "Statistics as rt_camera_rays (unchanged)"
                    obs.update(_stats(ctx))
            elif cls == "aovs_denoise":
                w, h = a["shape"]
                aov = ctx.aovs(w, h, camera(scene, a["cam"]), out=_to(a["mem"], np.zeros((h, w, 8), F32)), mode=2, spp=a["spp"], frame_seed=a["seed"])
                obs["aov"] = _bytes(aov)
                obs.update(_stats(ctx))
                rgb = noise_image(a["shape"], a["seed"])[0] if rgb_in is None else rgb_in
                obs["denoised"] = _bytes(ctx.denoise(_to(a["mem"], rgb), aov))
                obs["stats.denoise.pixels"] = ctx.stats()["pixels"]
            elif cls == "denoise":
                rgb, aov = noise_image(a["shape"], a["seed"])
                obs["denoised"] = _bytes(ctx.denoise(_to(a["mem"], rgb), _to(a["mem"], aov), iterations=1 + a["seed"] % 3))
                obs.update(_stats(ctx))
            elif cls == "reads":
                for what in a["order"]:
                    if what == "rgb32f":
                        obs[what] = _bytes(ctx.read_rgb32f())
                    elif what == "combined":
                        obs[what] = _bytes(ctx.read_rgba8_combined())
                    elif what == "channels":
                        obs[what] = b"".join(_bytes(c) for c in ctx.read_rgba8_channels())
                    else:
                        obs[what] = b"".join(_bytes(x) for x in ctx.read_hits())
            elif cls == "dispatch":
                w, h = a["shape"]
                sc = base_scene(scene)
                for off, size, channel in dispatch_jobs(a):
                    ctx.dispatch_tile(hostpack.push_constants((w, h), camera(scene, 0), len(sc.triangles), len(sc.materials), off, size,
                                                              hostpack.tile_count(w, h, a["tile"]), max(len(sc.triangles), 1),
                                                              np.zeros((), T.SCENE_METADATA_OFFSETS), channel, mode=a["mode"]))
                if a["read"] or not pending_ok:  # else the last dispatch stays in flight for the next operation
                    obs.update(_read_all(ctx, hits=True))
            elif cls == "rejected":
                _rejected(api, ctx, scene, a["kind"])
            else:
                raise KeyError(cls)
        except api.RtError as e:
            obs["code"] = e.code
        return obs

    # -- the fresh context ----------------------------------------------------------------------------------------------------------
    def fresh(self, r):
        ctx = self.api.Context()
        if r.scene is not None:
            ctx.upload_scene(scene_at(r.scene, r.pos, r.sph))
        return ctx

    def threshold(self, r):
        """The adaptive threshold of a running image: picked on a fresh context with the rule of test_gpu_adaptive._threshold (the 0.6
        quantile of the non-zero errors after MIN_SAMPLES samples)."""
        first = r.history[0] if r.history else r.op
        key = (r.scene, r.pos, r.sph, image_key(first))
        if key not in self.thresholds:
            with self.fresh(r) as ctx:
                for i in range(2):
                    assert self.execute(ctx, first, r.scene, threshold=0.0)["code"] == 0
                rec = ctx.read_adaptive()
            e = np_error(rec)
            e = e[np.isfinite(e) & (e > 0)]
            self.thresholds[key] = float(np.quantile(e, 0.6)) if e.size else 0.05  # (an empty scene: every error is 0)
        return self.thresholds[key]

    def reference(self, r, shapes):
        """What a fresh context answers for recipe `r` (memoised)."""
        if r in self.memo:
            return self.memo[r]
        thr = self.threshold(r) if r.op.cls == "adaptive" and r.scene is not None else 0.05
        with self.fresh(r) as ctx:
            for h in r.history:
                assert self.execute(ctx, h, r.scene, threshold=thr)["code"] == 0, h
            obs = self.execute(ctx, r.op, r.scene or shapes, threshold=thr)
        if r.op.cls == "adaptive" and obs["code"] == 0 and len(r.history) >= 2 and r.scene != "empty":
            n = np.frombuffer(obs["adaptive"], F32).reshape(-1, 8)[:, 3]
            n = n[n > 0]
            assert n.min() < n.max(), "the threshold must leave some pixels stopped and some running"
        self.memo[r] = obs
        return obs


def run_sequence(runner, name, ops, devices=(0,), env=None):
    """Every operation of `ops` on one warm context over `devices`, each held to the fresh context's answer; returns the number of
    comparisons made.  `env`: pytest's monkeypatch (RT_WF_BATCH / RT_WF_LANES of the warm context's frames)."""
    api = runner.api
    m = Model()
    compared, pending = 0, False
    with api.Context(devices) as ctx:
        for i, o in enumerate(ops):
            step = m.apply(o)
            where = f"{name}: operation {i} {o}\nsince the last upload:\n  " + "\n  ".join(f"{x.cls} {dict(x.args)}" for x in m.since_upload)
            r = step.recipe
            thr = runner.threshold(r) if o.cls == "adaptive" and m.scene is not None else 0.05
            rgb_in = None
            if o.cls == "aovs_denoise" and m.scene is not None and m.targets is not None and arg(m.targets.op)["shape"] == arg(o)["shape"]:
                rgb_in = np.frombuffer(runner.reference(m.targets, m.shapes)["rgb32f"], F32).reshape(arg(o)["shape"][1], arg(o)["shape"][0], 3)
            # "A call rejected for its arguments changes nothing": rt_stats included (not asked while a dispatch is pending: it would wait)
            quiet = o.cls == "rejected" and m.scene is not None and not pending
            before = _stats(ctx) if quiet else None
            got = runner.execute(ctx, o, m.shapes, rgb_in=rgb_in, threshold=thr, env=env, pending_ok=True)
            if quiet:
                assert _stats(ctx) == before, f"rt_stats changed over a rejected call\n{where}"
            pending = (o.cls == "dispatch" and not arg(o)["read"] and got["code"] == 0) or (pending and o.cls == "rejected")
            if step.code is not None:
                assert got["code"] == step.code, f"return code {got['code']}, the model says {step.code}\n{where}"
            if o.cls == "reads" and m.scene is not None:  # held to what the fresh context read when it had filled the targets
                want = dict(runner.reference(r, m.shapes), code=0) if r is not None else {"code": -4}
                if r is not None and "hits" not in want:  # rt_hip.h:207 the hit records are those of the last mode-0/1 frame
                    got.pop("hits", None)
            elif r is None:
                want = {}
            elif o.cls == "aovs_denoise" and rgb_in is not None:
                with runner.fresh(r) as ref:  # not memoised: the image to denoise is part of the warm context's history
                    want = runner.execute(ref, r.op, r.scene, rgb_in=rgb_in)
            else:
                want = runner.reference(r, m.shapes)
            for k in sorted(set(got) & set(want)):
                assert got[k] == want[k], f"{k} differs from the fresh context's" + (f": {got[k]} != {want[k]}" if not isinstance(got[k], bytes) else "") + f"\n{where}"
                compared += 1
            if not (o.cls == "dispatch" and not arg(o)["read"]):  # (rt_accumulated_samples does not wait; kept off a pending dispatch all the same)
                assert ctx.accumulated_samples() == step.samples, f"rt_accumulated_samples {ctx.accumulated_samples()}, the model says {step.samples}\n{where}"
            if step.check_tree and got["code"] == 0 and m.scene is not None:
                assert ctx.debug_check_bvh()["failures"] == 0, f"rt_debug_check_bvh reports failures\n{where}"
    return compared
