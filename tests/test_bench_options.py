"""bench.py's options (CPU): a plain run keeps only the headline inference, --full turns the other legs back on with
their usual defaults, and --steps / --warmup / --dump-outputs arrive as given."""
import bench
import pytest


@pytest.fixture(autouse=True)
def _no_full_in_the_environment(monkeypatch):
    monkeypatch.delenv("NRC_BENCH_FULL", raising=False)


def test_plain_run_turns_every_optional_leg_off():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert not a.full and a.dump_outputs is None
    assert a.no_cpu and a.no_wide and a.no_hash and a.no_c4 and a.no_peer
    assert a.sustained == 0 and a.frame_iters == 0
    # the legs' own options do not bring them back without --full
    b = bench.parse(["--sustained", "100", "--frame-iters", "5"])
    assert b.sustained == 0 and b.frame_iters == 0


def test_full_keeps_the_legs_and_their_options():
    a = bench.parse(["--full"])
    assert a.full
    assert not (a.no_cpu or a.no_wide or a.no_hash or a.no_c4 or a.no_peer)
    assert a.sustained == 4000 and a.frame_iters == 20 and a.train_frames == 20
    b = bench.parse(["--full", "--no-cpu", "--sustained", "0", "--dump-outputs", "d"])
    assert b.no_cpu and not b.no_wide and b.sustained == 0 and b.dump_outputs == "d"


def test_full_from_the_environment(monkeypatch):
    monkeypatch.setenv("NRC_BENCH_FULL", "1")
    a = bench.parse(["--steps", "5"])
    assert a.full and not a.no_cpu and a.sustained == 4000
    monkeypatch.setenv("NRC_BENCH_FULL", "0")
    assert not bench.parse([]).full
