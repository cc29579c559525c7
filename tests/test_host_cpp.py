"""The C++ host mirror (include/orbhip.hpp) driven by a compiled program, as the reference's
C++ host would call it: golden frame -> ORBextractor::operator() bit-exact; golden BA problem
-> Optimizer::LocalBundleAdjustment within 1e-4. The program is built by build() /
tests/cpp/Makefile; the CPU test only checks that it compiles and links against the C-ABI.
Two more programs need no library and no GPU: the staging block's offset allocator and the
extraction planner (plan invariants, and the ORBextractor ctor tables against the oracle)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "build", "host_adapter_check")
GOLD = os.path.join(ROOT, "tests", "golden")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP])
    assert os.path.exists(EXE)


def test_host_adapter_compiles_and_links():
    _build()


def test_stage_layout_offsets():
    """StageLayout (csrc/stage.h), host only: aligned non-decreasing offsets, zero-byte segments,
    hand-computed 16- and 256-byte layouts, the total as the aligned end."""
    _build()
    r = subprocess.run([os.path.join(CPP, "build", "stage_layout_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stage layout OK" in r.stdout


def _run_plan_check():
    _build()
    return subprocess.run([os.path.join(CPP, "build", "extract_plan_check")], capture_output=True, text=True,
                          timeout=120)


def test_extract_plan_invariants():
    """The extraction planner (csrc/extract_plan.cpp) as a host program: cone, band, flow, cell,
    octree and tap invariants of every shape and switch struct in tests/cpp/extract_plan_check.cpp,
    and which shapes return ORBHIP_ERR_UNSUPPORTED. 306x230 and 306x228 at 8 levels / 1.2 both
    have a last level of 64 rows, which passes the level-size check and fails the cell grid (32
    rows of cell area, under one 35-px cell row); 320x240 (67 rows) is the smallest that plans,
    316x237 (66 rows) does not."""
    r = _run_plan_check()
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    assert fails == [] and r.returncode == 0, "\n".join(fails) + "\n" + r.stdout[-300:]
    assert "extract plan OK" in r.stdout


def test_extract_plan_level_tables_match_oracle(oracle):
    """ORBextractor's constructor tables (level sizes, features per level, scale factors, umax) as
    the planner computes them against the oracle's, exactly: every shape of the program, whatever
    its level count, and nfeatures = 1250 at 640x480 against the values pinned in test_oracle_kats.py."""
    r = _run_plan_check()
    seen = {}
    for ln in r.stdout.splitlines():
        if not ln.startswith("levels "):
            continue
        head, *cols = [c.split() for c in ln[len("levels "):].split("|")]
        w, h, nfeat, sf, nlev = int(head[0]), int(head[1]), int(head[2]), np.float32(head[3]), int(head[4])
        assert [len(c) for c in cols] == [nlev] * 4 + [16], ln
        seen[(w, h, nfeat, nlev)] = cols
        o = oracle.level_info(w, h, nfeat, float(sf), nlev)
        assert [int(v) for v in cols[0]] == o["w"].tolist(), ln
        assert [int(v) for v in cols[1]] == o["h"].tolist(), ln
        assert [int(v) for v in cols[2]] == o["feats"].tolist(), ln
        assert np.array_equal(np.array(cols[3], np.float32), o["scales"]), ln
        assert [int(v) for v in cols[4]] == o["umax"].tolist(), ln
    for key in [(320, 240, 1000, 8), (641, 479, 1000, 8), (306, 230, 1000, 8), (306, 228, 1000, 8),
                (316, 237, 1000, 8), (640, 480, 1250, 8), (320, 240, 1000, 1), (641, 481, 1000, 5),
                (1001, 751, 1000, 3), (67, 67, 100, 1), (1000, 100, 500, 2), (640, 480, 1000, 9),
                (640, 480, 1000, 12), (4100, 99, 500, 1)]:
        assert key in seen, key
    c = seen[(640, 480, 1250, 8)]
    assert [int(v) for v in c[0]] == [640, 533, 444, 370, 309, 257, 214, 179]
    assert [int(v) for v in c[1]] == [480, 400, 333, 278, 231, 193, 161, 134]
    assert [int(v) for v in c[2]] == [271, 226, 189, 157, 131, 109, 91, 76]
    assert [int(v) for v in c[4]] == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def _unpack(d):
    z = np.load(os.path.join(GOLD, "frame_320x240_s5.npz"))
    z["image"].astype(np.uint8).tofile(os.path.join(d, "image.u8"))
    np.array([z["w"], z["h"], z["nfeatures"], z["lap"][0], z["lap"][1], z["mono"], len(z["kps"])],
             np.int32).tofile(os.path.join(d, "meta.i32"))
    z["kps"].astype(np.float32).tofile(os.path.join(d, "kps.f32"))
    z["desc"].astype(np.uint8).tofile(os.path.join(d, "desc.u8"))
    b = np.load(os.path.join(GOLD, "ba_10kf_200pt_s21.npz"))
    np.array(list(b["cam"]) + [float(b["huber_delta"]), float(b["iterations"])], np.float32).tofile(
        os.path.join(d, "ba_meta.f32"))
    for k, ext, dt in [("pose_q", "f32", np.float32), ("pose_t", "f32", np.float32), ("pose_fixed", "u8", np.uint8),
                       ("points", "f32", np.float32), ("edge_pose", "i32", np.int32), ("edge_point", "i32", np.int32),
                       ("edge_uv", "f32", np.float32), ("edge_octave", "i32", np.int32),
                       ("inv_sigma2", "f32", np.float32)]:
        np.ascontiguousarray(b[k], dt).tofile(os.path.join(d, f"ba_{k}.{ext}"))
    b["out_pose_t"].astype(np.float32).tofile(os.path.join(d, "ba_out_pose_t.f32"))
    b["out_points"].astype(np.float32).tofile(os.path.join(d, "ba_out_points.f32"))
    b["out_chi2"].astype(np.float64).tofile(os.path.join(d, "ba_out_meta.f64"))


@pytest.mark.gpu
def test_host_adapter_on_gpu(tmp_path):
    if not os.path.exists(EXE):
        _build()
    _unpack(str(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "orb_slam3_ros2_amd") + ":" +
               os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host adapter OK" in r.stdout
