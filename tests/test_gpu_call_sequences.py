"""A warm context answers as a fresh one does: the call sequences of tests/sequence_cases.py on the MI355X, one test per TRIPLES row and
one per random seed.  Every operation of a sequence is held, by bytes, to a fresh context that uploads the scene as it stands, replays the
running image's calls and runs the operation; a mismatch names the seed or row, the index of the operation and the operations since the
last upload.  The model, the sequences and the runner are in sequence_cases.py; what they cover is checked in test_sequence_cases.py."""
import pytest

try:
    import torch  # noqa: F401  (before any context exists: api.Context then brings torch's device runtime up first)
except ImportError:  # the device-memory operations then fail where they are run, not at collection
    torch = None

import sequence_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runner(rt_api):
    return sc.Runner(rt_api)  # the fresh contexts' answers, computed once and shared by every test below


@pytest.mark.parametrize("name", list(sc.TRIPLES))
def test_triple(runner, monkeypatch, name):
    compared = sc.run_sequence(runner, f"row {name}", sc.triple(name), env=monkeypatch)
    print(f"{name}: {compared} comparisons with fresh contexts")
    assert compared > 0


@pytest.mark.parametrize("seed", sc.RANDOM_SEEDS)
def test_random_sequence(runner, monkeypatch, seed):
    devices = (0, 0) if seed == sc.MULTI_DEVICE_SEED else (0,)
    compared = sc.run_sequence(runner, f"seed {seed}", sc.random_sequences()[seed], devices=devices, env=monkeypatch)
    print(f"seed {seed}: {compared} comparisons with fresh contexts")
    assert compared > 0


def test_quality_tree_leaves_the_last_frame_readable(runner):
    """Regression of the pair (a frame, rt_prepare(RT_PREPARE_QUALITY_TREE)) followed by rt_read_*: the quality tree of a device-built
    scene used to end the last frame (the reads answered RT_ERR_NOT_UPLOADED), while on a scene that already had the host builder's
    tree they kept answering; the tree in use must not show."""
    for scene in ("soup1200", "cornell12"):
        ops = [sc.U(scene), sc.F01(mode=1), sc.PT(), sc.RD(), sc.ACC(), sc.PT(), sc.RD(("hits", "combined", "rgb32f", "channels"))]
        assert sc.run_sequence(runner, f"frame, quality tree, reads on {scene}", ops) > 0
