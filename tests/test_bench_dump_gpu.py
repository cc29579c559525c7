"""bench.py --dump-outputs: a plain run (no --full) prints the headline line and writes what its
last timed step computed, one float32 .npy per output over the 16 cameras; the dumped keypoints,
descriptors and matches of a camera equal the oracle's on the frames that step pushed."""
import json
import os

import numpy as np
import pytest

STEPS, WARMUP = 3, 2


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path, capsys, oracle):
    import bench
    bench.main(["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    fps = 1e3 * line["config"]["frames_per_step"] / line["ms_per_step"]
    assert abs(line["value"] - fps) <= 1e-3 * fps
    assert not {"roofline", "extra", "cpu_baseline", "batch1_latency_ms"} & set(line)
    names = ("kps", "desc", "n", "mono", "match", "best", "second", "nmatch")
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    d = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and a.shape[0] == 16 for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    frames = bench.make_stream_frames(bench.FrontendC2.NF, bench.FrontendC2.W, bench.FrontendC2.H, 1)
    last = WARMUP + STEPS - 1
    for c in (0, 7):
        omono, ok, od = oracle.extract(frames[(last + 5 * c) % len(frames)])
        _, pk, pd = oracle.extract(frames[(last - 1 + 5 * c) % len(frames)])
        n = len(ok)
        assert d["n"][c, 0] == n and d["mono"][c, 0] == omono
        assert np.array_equal(d["kps"][c, :n], ok.astype(np.float32)) and np.array_equal(d["desc"][c, :n], od)
        assert not d["kps"][c, n:].any() and not d["desc"][c, n:].any()
        on, om, ob, os_ = oracle.match_bf(pd, pk[:, 3].astype(np.float32), od, ok[:, 3].astype(np.float32),
                                          50, 0.9, True)
        nq = len(pk)
        assert d["nmatch"][c, 0] == on and np.array_equal(d["match"][c, :nq], om[:nq])
        assert np.all(d["match"][c, nq:] == -1)
