"""What the CPU statement says about the frames of long_path_cases.py: the conditions under which test_gpu_long_paths.py takes the
queue pipeline through an early stop at its every-8th-bounce poll, past a first, second and third poll, and - with one sample per
batch - through both in one frame.  Nothing here touches the HIP library."""
import pytest

import long_path_cases as lp


@pytest.mark.parametrize("name", list(lp.SCENES))
def test_measured_constants_are_what_the_statement_gives(oracle_mod, name):
    got = {b: lp.cont(oracle_mod, name, b) for b in lp.MEASURE_AT}
    print(name, got)
    assert got == lp.MEASURED_CONT[name]
    assert {b: lp.poll_outcome(oracle_mod, name, b) for b in lp.BOUNCES[name]} == lp.MEASURED_POLLS[name]
    # cont(B) never shrinks with B, and every frame traces its camera segments
    seq = [got[b] for b in sorted(got)]
    assert seq == sorted(seq)
    assert lp.statement(oracle_mod, name, 8)["segments"]["camera"] == lp.W * lp.HT * lp.SPP


def test_open_scene_stops_at_its_first_poll(oracle_mod):
    """cont(8) == cont(7): no path starts bounce 8, so every batch of a frame with more than 7 bounces reads 0 at its first poll;
    cont(7) > cont(1): the frame is not trivially short."""
    c = {b: lp.cont(oracle_mod, "open", b) for b in (1, 7, 8)}
    assert c[8] == c[7] > c[1] > 0
    for b in lp.BOUNCES["open"]:
        assert lp.poll_outcome(oracle_mod, "open", b) == ((0, True) if b >= 8 else (0, False))
    assert all(b in lp.BOUNCES["open"] for b in lp.SPLIT_BOUNCES["open"])


def test_closed_bright_scene_goes_on_at_three_polls_and_stops_before_255(oracle_mod):
    c = {b: lp.cont(oracle_mod, "closed_bright", b) for b in (8, 9, 16, 17, 24, 25, 254, 255)}
    assert c[9] > c[8] and c[17] > c[16] and c[25] > c[24]
    assert c[255] == c[254]
    # the polls themselves read the paths that start bounces 8, 16, 24
    assert all(lp.starts(oracle_mod, "closed_bright", b) > 0 for b in (8, 16, 24))
    assert lp.poll_outcome(oracle_mod, "closed_bright", 17) == (2, False)   # an odd bounce count past the second poll
    assert lp.poll_outcome(oracle_mod, "closed_bright", 25)[0] == 3
    went_on, stopped = lp.poll_outcome(oracle_mod, "closed_bright", 255)
    assert stopped and went_on >= 3
    # the split variants' bounce counts have both outcomes between them
    outcomes = [lp.poll_outcome(oracle_mod, "closed_bright", b) for b in lp.SPLIT_BOUNCES["closed_bright"]]
    assert any(s for _, s in outcomes) and any(n > 0 and not s for n, s in outcomes)


def test_closed_dim_scene_stops_at_its_second_poll(oracle_mod):
    """cornell12 passes the first poll and reads 0 at the second: an early stop after an even number of polls, where the open scene's
    is after an odd one."""
    assert lp.starts(oracle_mod, "closed_dim", 8) > 0 and lp.starts(oracle_mod, "closed_dim", 16) == 0
    assert lp.poll_outcome(oracle_mod, "closed_dim", 17) == (1, True)


def test_one_sample_per_batch_mixes_both_outcomes_in_one_frame(oracle_mod):
    """closed_bright at 255 bounces with RT_WF_BATCH=1: at some poll one sample index has no path left while another has."""
    table = lp.alive_by_sample_group(oracle_mod, "closed_bright", 255)
    for b, row in table.items():
        print(b, dict(zip(lp.SAMPLE_GROUPS, row)))
    assert table == lp.MEASURED_MIXED
    mixed = [b for b, row in table.items() if any(v == 0 for v in row) and any(v > 0 for v in row)]
    assert mixed, "no poll at which one batch stops and another goes on"
    assert max(table) < 255 and not any(table[max(table)])   # every batch has stopped early by then
    # per poll the groups add up to the whole frame's figure
    for b, row in table.items():
        assert sum(row) == lp.starts(oracle_mod, "closed_bright", b)
