"""The call sequences of tests/sequence_cases.py, checked without a device: the generators are deterministic, every operation is legal
in the model state it meets, the TRIPLES table covers every state group with existing classes, the eight random sequences together
contain every ordered pair of operation classes, and nothing comes before a sequence's first upload."""
import numpy as np
import pytest

import sequence_cases as sc


def _all_sequences():
    for name in sc.TRIPLES:
        yield name, sc.triple(name)
    for seed, ops in sc.random_sequences().items():
        yield f"seed {seed}", ops


def test_generators_are_deterministic():
    first = {seed: list(ops) for seed, ops in sc.random_sequences().items()}
    sc.random_sequences.cache_clear()
    again = sc.random_sequences()
    assert list(first) == list(sc.RANDOM_SEEDS) == list(again)
    for seed in sc.RANDOM_SEEDS:
        assert first[seed] == again[seed], seed
    rows = {name: sc.triple(name) for name in sc.TRIPLES}
    assert rows == {name: sc.triple(name) for name in sc.TRIPLES}
    assert sc._pending_rows() == sc._pending_rows()
    # the seeds differ from one another, and an operation is a plain value: hashable and equal to its copy
    assert len({tuple(ops) for ops in first.values()}) == len(sc.RANDOM_SEEDS)
    assert sc.F2() == sc.F2() and hash(sc.F2()) == hash(sc.F2()) and sc.F2() != sc.F2(spp=3)
    # inputs come from the scene's box and a seed, and nothing else
    a, b = sc.query_input("soup1200", "rays", 65, 3), sc.query_input("soup1200", "rays", 65, 4)
    assert a.shape == (65, 8) and a.dtype == np.float32 and not np.array_equal(a, b)
    sc.query_input.cache_clear()
    assert np.array_equal(a, sc.query_input("soup1200", "rays", 65, 3))
    assert np.array_equal(sc.positions("soup1200", ("rigid", 2)), sc.positions("soup1200", ("rigid", 2)))
    assert not np.array_equal(sc.positions("soup1200", ("rigid", 2)), sc.positions("soup1200", ("jitter", 2)))


def test_every_operation_is_legal_in_the_state_it_meets():
    for name, ops in _all_sequences():
        m = sc.Model()
        for i, o in enumerate(ops):
            assert o.cls in sc.CLASSES, (name, i, o)
            assert m.legal(o), (name, i, o)
            before = m.scene
            step = m.apply(o)
            a = sc.arg(o)
            if o.cls == "failed_upload":
                assert step.code == -2 and m.scene is None
            elif before is None and o.cls != "upload":
                # a context without a scene: the fresh context's code decides (RT_ERR_NOT_UPLOADED for all but what needs no scene)
                assert step.code is None and step.recipe.scene is None and m.image is None and m.targets is None
            elif o.cls == "rejected":
                assert step.code == -1
            else:
                assert step.code == (-4 if o.cls == "reads" and m.targets is None else 0), (name, i, o)
            # shapes stay within what the issue allows
            if "shape" in a:
                assert a["shape"] in sc.SHAPES
            if "spp" in a:
                assert 1 <= a["spp"] <= (8 if o.cls == "aovs_denoise" else 5)
            if o.cls in ("frame2", "accumulate", "accumulate_restart", "adaptive"):
                assert 0 <= a["bounces"] <= 3 and a["tile"] in (0, 16, 32) and a["variant"] in sc.VARIANTS
                assert a["wf_batch"] in (None, 1, 3) and a["wf_lanes"] in (None, 1, 2)
            if o.cls == "batch":
                assert a["kind"] in sc.BATCH_KINDS and (a["n"] in sc.BATCH_SIZES or o == sc.full_check()[2])
            # a continued running image is continued under its own key
            if m.image:
                assert all(sc.image_key(c) == m.image[0] for c in m.image[1])
                assert m.samples() == sum(sc.arg(c)["spp"] for c in m.image[1]) <= 64
        assert ops[-3:] == sc.full_check() and m.scene is not None, name


def test_the_model_ends_and_keeps_the_running_image_as_the_header_says():
    m = sc.Model()
    m.apply(sc.U("soup1200"))
    assert m.apply(sc.ACC(spp=2)).samples == 2 and m.apply(sc.ACC(spp=3)).samples == 5
    for keeps in (sc.PT(), sc.PG(), sc.B("intersect"), sc.AOVD(), sc.DN(), sc.RD(), sc.REJ("render_bounces")):
        assert m.apply(keeps).samples == 5, keeps  # rt_hip.h: "It survives rt_prepare, ... the ray queries, ... rt_denoise, rt_get_stats and rt_read_*"
    assert m.apply(sc.ACC(spp=1, variant="kernel_sm", wf_lanes=1)).samples == 6  # "The other RT_FLAG_* bits change no bits and may differ"
    for changed in (dict(seed=4), dict(shape=(37, 29)), dict(bounces=1), dict(tile=32), dict(share=True), dict(cam=1)):
        assert m.apply(sc.ACC(spp=1, **changed)).samples == 1, changed  # another key: a new image by itself
        assert m.apply(sc.ACC(spp=1, **changed)).samples == 2
    assert m.apply(sc.ACC(spp=1, tile=0)).samples == 1 and m.apply(sc.ACC(spp=2, restart=True)).samples == 2
    assert m.apply(sc.AD()).samples == 2 and m.apply(sc.AD()).samples == 4 and m.apply(sc.ACC()).samples == 2  # plain after adaptive, and the reverse
    for ends in (sc.U("soup1200"), sc.UH("jitter", 1), sc.UD("jitter", 1), sc.US(1), sc.UR("jitter", 1), sc.DISP(), sc.F2(), sc.F01(), sc.FAIL("empty")):
        if m.scene is None:
            m.apply(sc.U("soup1200"))
        assert m.apply(sc.ACC(spp=2, restart=True)).samples == 2 and m.apply(sc.ACC(spp=2)).samples == 4
        assert m.apply(ends).samples == 0 and m.image is None, ends
    # the targets: gone with an upload, left alone by updates, queries and rt_prepare
    m.apply(sc.U("cornell12"))
    assert m.targets is None and m.apply(sc.RD()).code == -4
    t = m.apply(sc.F01()).recipe
    for o in (sc.UH("rigid", 1), sc.PT(), sc.PG(), sc.B("occluded"), sc.DN(), sc.REJ("aovs_mode"), sc.US(1)):
        m.apply(o)
        assert m.targets == t and m.apply(sc.RD()).recipe == t
    assert t.pos is None and m.pos == ("rigid", 1)  # ... and they hold the frame of the positions it was rendered with


def test_triples_name_existing_classes_and_cover_every_state_group():
    groups = {}
    for name, (group, ops) in sc.TRIPLES.items():
        assert group in sc.STATE_GROUPS and 3 <= len(ops) <= 6, name
        assert all(o.cls in sc.CLASSES for o in ops), name
        assert ops[0].cls == "upload", name
        groups.setdefault(group, []).append(name)
    assert set(groups) == set(sc.STATE_GROUPS)
    cls_of = lambda name: [o.cls for o in sc.TRIPLES[name][1]]
    has = lambda group, *classes: any(all(c in cls_of(n) for c in classes) for n in groups[group])
    # light grids: every ender after something that builds them, the spheres-only update that keeps them, every user
    for ender in ("update_host", "update_device", "update_rebuild", "prepare_tree", "upload", "update_spheres"):
        assert any(ender in cls_of(n)[1:] for n in groups["grids"]), ender
    assert has("grids", "prepare_grids") and has("grids", "frame2") and has("grids", "accumulate") and has("grids", "adaptive")
    assert any(sc.arg(o).get("kind") == "direct_light" for n in groups["grids"] for o in sc.TRIPLES[n][1])
    beams = [sc.arg(o) for n in groups["beams"] for o in sc.TRIPLES[n][1] if o.cls == "frame2"]
    assert {b["cam"] for b in beams} == {0, 1} and len({b["shape"] for b in beams}) > 1 and {b["tile"] for b in beams} >= {0, 16, 32}
    assert any(b["share"] for b in beams) and has("beams", "upload", "update_host")
    assert has("refit", "prepare_tree", "update_host") and has("refit", "update_rebuild", "update_host")
    assert any(cls_of(n).count("upload") == 2 for n in groups["refit"])
    for reader in ("prepare_tree", "prepare_grids", "frame2", "update_rebuild", "update_host"):
        assert any(cls_of(n)[1] == "update_device" and reader in cls_of(n)[2:] for n in groups["mirror"]), reader
    pipe = [[sc.arg(o) for o in sc.TRIPLES[n][1] if o.cls == "frame2"] for n in groups["pipeline"]]
    assert any([f["wf_lanes"] for f in fs] == [2, 1, 2] for fs in pipe) and any([f["wf_batch"] for f in fs][:2] == [3, None] for fs in pipe)
    assert any(len({f["spp"] for f in fs}) >= 3 for fs in pipe) and any(cls_of(n).count("upload") >= 2 for n in groups["pipeline"])
    assert has("targets", "dispatch", "reads") and any(len({sc.arg(o)["shape"] for o in sc.TRIPLES[n][1] if "shape" in sc.arg(o)}) > 1 for n in groups["targets"])
    assert has("sums", "accumulate") and has("sums", "adaptive")
    assert [sc.arg(o)["tile"] for o in sc.TRIPLES["sums_adaptive_cap_grows"][1][1:]] == [16, 16, 32, 0, 0]  # 48, 64 and 256 blocks of 64x48
    st = [[(sc.arg(o)["kind"], sc.arg(o)["n"]) for o in sc.TRIPLES[n][1][1:]] for n in groups["staging"]]
    assert [("intersect", 130), ("intersect", 65)] == st[0][:2] and any(s[:2] == [("ambient_occlusion", 130), ("ambient_occlusion", 65)] for s in st)
    assert any([k for k, _ in s[:3]] == ["intersect_all", "overlap_box", "inside"] for s in st)
    dn = [sc.arg(o)["shape"] for o in sc.TRIPLES["denoiser_96x64_then_37x29"][1] if o.cls == "denoise"]
    assert dn == [(96, 64), (37, 29)]
    cnt = sc.TRIPLES["counters_frame__query__path_query__plain_frame"][1]
    assert sc.arg(cnt[1])["counters"] and sc.arg(cnt[2])["counters"] and sc.arg(cnt[3])["kind"] == "radiance" and cnt[-1].cls == "frame01"
    # a pending dispatch before each operation class
    for cls in sc.CLASSES:
        ops = sc.TRIPLES[f"pending_dispatch__{cls}"][1]
        assert ops[-2].cls == "dispatch" and not sc.arg(ops[-2])["read"] and ops[-1].cls == cls
    assert has("errors", "rejected") and has("errors", "failed_upload")
    assert {sc.arg(o)["kind"] for n in groups["errors"] for o in sc.TRIPLES[n][1] if o.cls == "rejected"} >= {"render_bounces", "update_count", "query_flags"}


def test_random_sequences_contain_every_ordered_pair_of_classes():
    seqs = sc.random_sequences()
    assert len(seqs) == 8 and sc.MULTI_DEVICE_SEED in seqs
    covered = set()
    for ops in seqs.values():
        assert len(ops) <= sc.RANDOM_LENGTH + 1 + len(sc.full_check())
        covered |= sc.adjacent_pairs(ops)
    missing = sorted((a, b) for a in sc.CLASSES for b in sc.CLASSES if (a, b) not in covered)
    assert not missing, missing
    # every batch call, rejected call, kernel variant and scene appears somewhere in the sequences
    everything = [o for _, ops in _all_sequences() for o in ops]
    assert {sc.arg(o)["kind"] for o in everything if o.cls == "batch"} == set(sc.BATCH_KINDS)
    assert {sc.arg(o)["kind"] for o in everything if o.cls == "rejected"} == set(sc.REJECTED_KINDS)
    assert {sc.arg(o)["variant"] for o in everything if o.cls == "frame2"} == set(sc.VARIANTS)
    assert {sc.arg(o)["scene"] for o in everything if o.cls == "upload"} == set(sc.SCENE_NAMES)
    assert {(sc.arg(o)["mem"], sc.arg(o)["counters"]) for o in everything if o.cls == "batch"} == {(m, c) for m in ("host", "device") for c in (False, True)}


def test_nothing_comes_before_the_first_upload():
    for name, ops in _all_sequences():
        assert ops[0].cls == "upload", name  # (rt_hip.h allows the ray generators, rt_denoise and rt_upload_textures before it; no sequence uses that)
        steps, _ = sc.run_model(ops)
        assert steps[0].code == 0


@pytest.mark.parametrize("kind", sorted(set(sc.INPUT_OF.values())))
def test_query_inputs_have_the_records_shape(kind):
    cols = {"rays": 8, "surface": 8, "points": 4, "probes": 4, "sweeps": 8, "boxes": 8, "obbs": 12, "box_sweeps": 12, "obb_sweeps": 16, "capsules": 8,
            "capsule_sweeps": 12}[kind]
    for scene in sc.SCENE_NAMES:
        for n in sc.BATCH_SIZES:
            x = sc.query_input(scene, kind, n, 1)
            assert x.shape == (n, cols) and x.dtype == np.float32 and x.flags.c_contiguous and np.isfinite(x[:, :3]).all()
