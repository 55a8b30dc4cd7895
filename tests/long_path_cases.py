"""Extended-mode frames whose paths live past the queue pipeline's every-8th-bounce poll, and what the CPU statement says about them.

After bounce iterations 7, 15, 23, ... (never after the last one) the pipeline reads back how many paths go on; a batch that reads 0
ends there, at whatever bounce parity it has reached, and any other goes on.  With cont(B) the continuation segments of the frame at
max_bounces = B, cont(B) - cont(B - 1) paths start bounce B (a path's walk up to its vertex B - 1 does not depend on max_bounces: only
the terminal vertex is shaded differently, and nothing follows it), so the poll after iteration 8p - 1 of a batch that holds the whole
frame reads cont(8p) - cont(8p - 1).

Three scenes, chosen for how long their paths live:
  open           the triangle soup of test_gpu_path_compaction.py under the sky: paths leave within a few bounces
  closed_dim     cornell12 (albedo <= 0.73, open toward the camera)
  closed_bright  a closed unit box, camera inside, one point light: diffuse walls whose largest albedo channel is 0.95 and one rough
                 metallic wall.  From the third vertex on a path survives with p = clamp(max(throughput), 0.05, 1) and its throughput
                 is divided by p, so after the first roulette step the largest channel is 1 and the next
                 vertex leaves it at about the largest albedo channel: a path goes on with probability of roughly 0.95 per vertex,
                 less what the metallic wall absorbs (directions that point into it, step 4).

Everything here comes from oracle.render_extended (brute force, no tree); nothing is measured on a HIP result.  The MEASURED_*
constants record what the statement gave when this module was written; test_long_paths_oracle.py recomputes and compares them, and
asserts the conditions that make test_gpu_long_paths.py mean something."""
import numpy as np

import estimator_cases as ec
from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import scenes

W, HT, SPP, FRAME_SEED = 45, 27, 6, 5   # ragged: 6 x 4 pixel blocks of 8 x 8, the last column and row partly outside

ALL_BOUNCES = (7, 8, 9, 15, 16, 17, 24, 25, 64, 255)
BOUNCES = {"open": (7, 8, 9, 15, 16, 17, 255), "closed_dim": ALL_BOUNCES, "closed_bright": ALL_BOUNCES}
# bounce counts of the work-splitting variants: both poll outcomes occur (MEASURED_POLLS)
SPLIT_BOUNCES = {"open": (9,), "closed_dim": (17,), "closed_bright": (17, 255)}
MEASURE_AT = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 64, 254, 255)


def _open():
    return scenes.random_soup(300, seed=5, size=0.6, n_spheres=3, n_lights=3)


BRIGHT_WHITE, BRIGHT_WARM, BRIGHT_COOL, BRIGHT_METAL = (0.95, 0.95, 0.95), (0.95, 0.9, 0.85), (0.85, 0.9, 0.95), (0.95, 0.93, 0.9)


def _closed_bright():
    """The furnace's unit box and camera (estimator_cases.furnace), its six faces wound to face inward so that the point light
    reaches them (step 2 uses the unflipped geometric normal): floor, ceiling and back wall white, left warm, right cool, the
    wall behind the camera metallic with roughness 0.4."""
    mesh = ec._Mesh()
    ec._quad(mesh, (0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), 0, (0, 1, 0))     # floor
    ec._quad(mesh, (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1), 0, (0, -1, 0))    # ceiling
    ec._quad(mesh, (0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), 0, (0, 0, 1))     # back wall z = 0 (the camera looks at it)
    ec._quad(mesh, (0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), 1, (1, 0, 0))     # left
    ec._quad(mesh, (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0), 2, (-1, 0, 0))    # right
    ec._quad(mesh, (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1), 3, (0, 0, -1))    # behind the camera
    mats = [H.material_diffuse(BRIGHT_WHITE), H.material_diffuse(BRIGHT_WARM), H.material_diffuse(BRIGHT_COOL),
            H.material_metallic(BRIGHT_METAL, 0.4)]
    cam = H.camera((0.37, 0.45, 0.81), tuple(ec._unit((0.2, -0.1, -1.0))), (0.0, 1.0, 0.0), 70.0)
    light = H.light_point((0.6, 0.8, 0.4), (1.0, 0.95, 0.9), 0.5)
    return ec._scene("closed_bright", mesh, mats, cam, [light])


SCENES = {"open": _open, "closed_dim": scenes.cornell12, "closed_bright": _closed_bright}

_SCENE_CACHE, _STATEMENT = {}, {}


def scene(name):
    if name not in _SCENE_CACHE:
        _SCENE_CACHE[name] = SCENES[name]()
    return _SCENE_CACHE[name]


def statement(oracle_mod, name, bounces, spp=SPP):
    """The CPU statement's frame (rgb, segments) of scene `name` at `bounces`, rendered once per session and left unchanged."""
    key = (name, bounces, spp)
    if key not in _STATEMENT:
        out = oracle_mod.render_extended(oracle_mod.PackedScene(scene(name), use_bvh=False), W, HT, spp, bounces, frame_seed=FRAME_SEED)
        out["rgb"].setflags(write=False)
        _STATEMENT[key] = out
    return _STATEMENT[key]


def cont(oracle_mod, name, bounces, spp=SPP):
    return statement(oracle_mod, name, bounces, spp)["segments"]["continuation"]


def starts(oracle_mod, name, bounce, spp=SPP):
    """Paths of the spp-sample frame that start bounce `bounce` (>= 1)."""
    return cont(oracle_mod, name, bounce, spp) - cont(oracle_mod, name, bounce - 1, spp)


def polls_of(max_bounces):
    """The bounces 8, 16, ... whose starting paths a frame of max_bounces polls (after iterations 7, 15, ... below max_bounces)."""
    return [it + 1 for it in range(7, max_bounces, 8)]


def poll_outcome(oracle_mod, name, max_bounces, spp=SPP):
    """-> (times a one-batch frame goes on at a poll, whether it then stops early at one)."""
    went_on = 0
    for b in polls_of(max_bounces):
        if starts(oracle_mod, name, b, spp) == 0:
            return went_on, True
        went_on += 1
    return went_on, False


SAMPLE_GROUPS = ("0+1", "2", "3", "4", "5")


def alive_by_sample_group(oracle_mod, name, max_bounces):
    """{polled bounce: paths starting it per sample group}, until no group has any.

    The statement renders samples 0 .. spp-1 of a frame and jitters them when spp > 1, so sample s >= 2 of the 6-spp frame is the
    (s+1)-spp frame less the s-spp frame (same seeds, same jitter); samples 0 and 1 come only together, as the 2-spp frame (the
    1-spp frame does not jitter).  With RT_WF_BATCH=1 every sample index is a batch of its own: a group that reads 0 at a poll
    stops there, 'none alive' for the pair means both of its batches stop, 'some alive' that at least one goes on."""
    table = {}
    for b in polls_of(max_bounces):
        per_spp = [starts(oracle_mod, name, b, spp) for spp in range(2, SPP + 1)]
        row = tuple([per_spp[0]] + [per_spp[k] - per_spp[k - 1] for k in range(1, len(per_spp))])
        table[b] = row
        if not any(row):
            break
    return table


# ---- what the statement gave (CPU only; test_long_paths_oracle.py recomputes every figure) ------------------------------------
# cont(B) of the 45 x 27, 6-spp frame with frame_seed 5, for B in MEASURE_AT
MEASURED_CONT = {
    "open": {1: 701, 7: 857, 8: 857, 9: 857, 15: 857, 16: 857, 17: 857, 23: 857, 24: 857, 25: 857, 64: 857, 254: 857, 255: 857},
    "closed_dim": {1: 4397, 7: 9028, 8: 9045, 9: 9052, 15: 9056, 16: 9056, 17: 9056, 23: 9056, 24: 9056, 25: 9056, 64: 9056, 254: 9056, 255: 9056},
    "closed_bright": {1: 7290, 7: 40919, 8: 45122, 9: 49017, 15: 67239, 16: 69567, 17: 71731, 23: 81825, 24: 83121, 25: 84329, 64: 98797, 254: 99458, 255: 99458},
}
# (polls passed with paths alive, stopped early at the next) per scene and max_bounces, from MEASURED_CONT's differences
MEASURED_POLLS = {
    "open": {7: (0, False), 8: (0, True), 9: (0, True), 15: (0, True), 16: (0, True), 17: (0, True), 255: (0, True)},
    "closed_dim": {7: (0, False), 8: (1, False), 9: (1, False), 15: (1, False), 16: (1, True), 17: (1, True), 24: (1, True), 25: (1, True), 64: (1, True), 255: (1, True)},
    "closed_bright": {7: (0, False), 8: (1, False), 9: (1, False), 15: (1, False), 16: (2, False), 17: (2, False), 24: (3, False), 25: (3, False), 64: (8, False), 255: (15, True)},
}
# closed_bright at 255 bounces, one sample index per batch: paths starting the polled bounce per SAMPLE_GROUPS, from the first poll at
# which a group has none to the poll at which no group has any
MEASURED_MIXED = {
    8: (1400, 688, 731, 692, 692),
    16: (774, 355, 406, 397, 396),
    24: (442, 193, 235, 227, 199),
    32: (244, 98, 121, 128, 110),
    40: (136, 57, 64, 69, 54),
    48: (76, 38, 40, 38, 23),
    56: (37, 18, 25, 21, 13),
    64: (16, 10, 19, 8, 4),
    72: (7, 7, 9, 4, 3),
    80: (2, 3, 4, 1, 2),
    88: (1, 1, 3, 1, 2),
    96: (1, 1, 2, 0, 1),
    104: (1, 0, 0, 0, 1),
    112: (1, 0, 0, 0, 1),
    120: (0, 0, 0, 0, 1),
    128: (0, 0, 0, 0, 0),
}
