"""Seeded synthetic inputs — no datasets exist offline.

Images: background 128, 300 axis-aligned rectangles (side U[8,96] px, intensity
U[0,255]) drawn in order, then Gaussian noise sigma=4, rounded and clipped to u8.
numpy PCG64 seeded with the frame index. This gives FAST corners in every 35-px
cell, like a textured indoor scene.
"""
from __future__ import annotations

import numpy as np


def synthetic_frame(seed: int, width: int = 640, height: int = 480, n_rect: int = 300,
                    noise_sigma: float = 4.0) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    img = np.full((height, width), 128.0, dtype=np.float64)
    for _ in range(n_rect):
        sw, sh = rng.integers(8, 97, size=2)
        x0 = int(rng.integers(-int(sw) + 1, width))
        y0 = int(rng.integers(-int(sh) + 1, height))
        val = float(rng.integers(0, 256))
        img[max(y0, 0):max(min(y0 + sh, height), 0), max(x0, 0):max(min(x0 + sw, width), 0)] = val
    if noise_sigma > 0:
        img += rng.normal(0.0, noise_sigma, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def synthetic_batch(first_seed: int, batch: int, width: int, height: int) -> np.ndarray:
    return np.stack([synthetic_frame(first_seed + i, width, height) for i in range(batch)])


def shifted_frame(base: np.ndarray, dx: int, dy: int, seed: int, noise_sigma: float = 2.0) -> np.ndarray:
    """A second view of ``base``: integer translation (edge-replicated) plus fresh noise,
    so consecutive frames share most corners (matcher workloads)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h, w = base.shape
    ys = np.clip(np.arange(h) - dy, 0, h - 1)
    xs = np.clip(np.arange(w) - dx, 0, w - 1)
    img = base[ys][:, xs].astype(np.float64)
    img += rng.normal(0.0, noise_sigma, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def synthetic_stream(n: int, width: int, height: int, seed0: int, noise_sigma: float = 4.0,
                     margin=(256, 128)) -> np.ndarray:
    """A camera panning over one static scene (SURVEY.md 8d image spec at every frame): the scene
    is a (width + mx) x (height + my) image with the 640x480 rectangle density (300 per 640x480),
    frame i the crop at a smooth offset (2-4 px right, 0-1 px down per frame, bouncing inside the
    margin) plus fresh N(0, noise_sigma) noise. Consecutive frames share most corners, and every
    frame has the same statistics (noise does not accumulate along the stream)."""
    mx, my = margin
    W, H = width + mx, height + my
    n_rect = int(round(300 * (W * H) / (640 * 480)))
    world = synthetic_frame(seed0, W, H, n_rect=n_rect, noise_sigma=0.0).astype(np.float64)
    rng = np.random.Generator(np.random.PCG64(seed0 + 1))
    out = np.empty((n, height, width), np.uint8)
    ox = oy = 0
    for i in range(n):
        img = world[oy:oy + height, ox:ox + width] + rng.normal(0.0, noise_sigma, size=(height, width))
        out[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        ox += 2 + (i % 3)
        oy += i % 2
        if ox > mx:
            ox = ox % (mx + 1)
        if oy > my:
            oy = oy % (my + 1)
    return out


def synthetic_stereo_pair(seed: int, width: int = 640, height: int = 480, n_rect: int = 300,
                          noise_sigma: float = 4.0, max_disparity: float = 24.0):
    """A rectified stereo pair of the rectangle scene (SURVEY.md 8d image spec): (left, right) u8.
    Every rectangle has its own disparity, a multiple of a quarter pixel in [0, max_disparity];
    the rectangles are drawn in order of increasing disparity, so nearer ones are drawn later and
    shifted further (x_right = x_left - disparity). The background has disparity 0. The right image
    is rendered at 4x width and box-averaged down, which gives the non-integer disparities their
    blended edges. Both images get fresh N(0, noise_sigma) noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    left = np.full((height, width), 128.0, dtype=np.float64)
    right4 = np.full((height, 4 * width), 128.0, dtype=np.float64)
    quarters = np.sort(rng.integers(0, int(4 * max_disparity) + 1, size=n_rect))
    for q in quarters:
        sw, sh = rng.integers(8, 97, size=2)
        x0 = int(rng.integers(-int(sw) + 1, width))
        y0 = int(rng.integers(-int(sh) + 1, height))
        val = float(rng.integers(0, 256))
        ya, yb = max(y0, 0), max(min(y0 + int(sh), height), 0)
        left[ya:yb, max(x0, 0):max(min(x0 + int(sw), width), 0)] = val
        xa, xb = 4 * x0 - int(q), 4 * (x0 + int(sw)) - int(q)
        right4[ya:yb, max(xa, 0):max(min(xb, 4 * width), 0)] = val
    right = right4.reshape(height, width, 4).mean(axis=2)
    if noise_sigma > 0:
        left += rng.normal(0.0, noise_sigma, size=left.shape)
        right += rng.normal(0.0, noise_sigma, size=right.shape)
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)   # noqa: E731
    return to_u8(left), to_u8(right)


# ---------------------------------------------------------------------------
# Bundle-adjustment problems
# ---------------------------------------------------------------------------
D435I = dict(fx=614.67, fy=617.63, cx=326.22, cy=245.58, w=640, h=480)   # R:config/Monocular/RealSense_D435i.yaml:16-29


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _mat_to_quat(R):
    """(x, y, z, w), w >= 0."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        w, x, y, z = 0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(3)
        q[i] = 0.25 * s
        w = (R[k, j] - R[j, k]) / s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
        x, y, z = q
    q = np.array([x, y, z, w])
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def _look_at(c, target=np.zeros(3)):
    """Rcw for a camera at c looking at target (camera z forward, y down)."""
    z = target - c
    z /= np.linalg.norm(z)
    up = np.array([0.0, -1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])   # rows: camera axes in world


def synthetic_ba_problem(n_kf=50, n_pts=2000, obs_per_pt=4, seed=7, layout="arc", window=None,
                         rot_noise=0.01, trans_noise=0.02, pt_noise=0.05, n_levels=8, scale_factor=1.2):
    """C4 (layout='arc'): KFs on a 2 m-radius arc looking inward, points uniform in a 1 m cube at
    the centre, each point seen by `obs_per_pt` distinct KFs. C5 (layout='loop'): KFs around a full
    circle, each point observed from a `window`-KF sliding window (co-visibility band).
    Returns (BAProblem with perturbed initial state, ground-truth dict)."""
    from .optimizer import BAProblem, TH_HUBER_MONO
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = D435I
    if layout == "arc":
        ang = np.linspace(-np.pi / 3, np.pi / 3, n_kf)
        radius = 2.0
    else:
        ang = np.linspace(0, 2 * np.pi, n_kf, endpoint=False)
        radius = 4.0
    Rs, ts = [], []
    for a in ang:
        c = np.array([radius * np.sin(a), 0.3 * np.sin(3 * a), -radius * np.cos(a)])
        R = _look_at(c)
        Rs.append(R)
        ts.append(-R @ c)
    Rs, ts = np.array(Rs), np.array(ts)
    pts = rng.uniform(-0.5, 0.5, size=(n_pts, 3))
    edges_pose, edges_pt = [], []
    for m in range(n_pts):
        if window is None:
            kfs = rng.choice(n_kf, obs_per_pt, replace=False)
        else:
            start = int(rng.integers(0, n_kf))
            kfs = (start + rng.choice(window, obs_per_pt, replace=False)) % n_kf
            # place the point where that window looks (in front of its middle keyframe)
            mid = (start + window // 2) % n_kf
            cmid = -Rs[mid].T @ ts[mid]
            pts[m] = cmid * 0.55 + rng.uniform(-0.4, 0.4, size=3)
        for k in sorted(kfs.tolist()):
            edges_pose.append(k)
            edges_pt.append(m)
    edges_pose = np.array(edges_pose, np.int32)
    edges_pt = np.array(edges_pt, np.int32)
    E = len(edges_pose)
    octave = rng.integers(0, n_levels, size=E).astype(np.int32)
    scales = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        scales[i] = np.float32(np.float64(scales[i - 1]) * np.float64(np.float32(scale_factor)))
    inv_sigma2 = (np.float32(1.0) / (scales * scales)).astype(np.float32)
    Xc = np.einsum("eij,ej->ei", Rs[edges_pose], pts[edges_pt]) + ts[edges_pose]
    uv = np.stack([cam["fx"] * Xc[:, 0] / Xc[:, 2] + cam["cx"], cam["fy"] * Xc[:, 1] / Xc[:, 2] + cam["cy"]], 1)
    sig = np.power(np.float64(scale_factor), octave)
    uv += rng.normal(size=uv.shape) * sig[:, None]
    # perturbed initial state (KF0 stays at ground truth and is fixed)
    q0, t0 = [], []
    for k in range(n_kf):
        if k == 0:
            R, t = Rs[k], ts[k]
        else:
            R = _rodrigues(rng.normal(size=3) * rot_noise) @ Rs[k]
            t = ts[k] + rng.normal(size=3) * trans_noise
        q0.append(_mat_to_quat(R))
        t0.append(t)
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    p0 = pts + rng.normal(size=pts.shape) * pt_noise
    prob = BAProblem(np.array(q0, np.float32), np.array(t0, np.float32), fixed, p0.astype(np.float32), edges_pose,
                     edges_pt, uv.astype(np.float32), octave, inv_sigma2, np.float32(cam["fx"]),
                     np.float32(cam["fy"]), np.float32(cam["cx"]), np.float32(cam["cy"]), TH_HUBER_MONO, 10, 0)
    gt = dict(R=Rs, t=ts, points=pts)
    return prob, gt


def synthetic_pose_problem(n=600, outlier_frac=0.15, seed=3, rot_noise=0.02, trans_noise=0.05, n_levels=8,
                           scale_factor=1.2):
    """A tracked monocular Frame for PoseOptimization: a camera looking at map points 2-6 m away,
    keypoints = projections + 1.2^octave px noise, a fraction replaced by gross mismatches
    (uniform in the image), initial pose perturbed like a constant-velocity prediction.
    Returns (PoseProblem, ground truth dict)."""
    from .optimizer import PoseProblem
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = D435I
    R = _rodrigues(rng.normal(size=3) * 0.3)
    t = rng.normal(size=3) * 0.5
    # points in front of the camera, inside the image
    z = rng.uniform(2.0, 6.0, size=n)
    u = rng.uniform(20, 620, size=n)
    v = rng.uniform(20, 460, size=n)
    Xc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1)
    Xw = (Xc - t) @ R          # R^T (Xc - t)
    octave = rng.integers(0, n_levels, size=n).astype(np.int32)
    scales = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        scales[i] = np.float32(np.float64(scales[i - 1]) * np.float64(np.float32(scale_factor)))
    inv_sigma2 = (np.float32(1.0) / (scales * scales)).astype(np.float32)
    uv = np.stack([u, v], 1) + rng.normal(size=(n, 2)) * np.power(np.float64(scale_factor), octave)[:, None]
    bad = rng.random(n) < outlier_frac
    uv[bad] = np.stack([rng.uniform(0, 640, bad.sum()), rng.uniform(0, 480, bad.sum())], 1)
    R0 = _rodrigues(rng.normal(size=3) * rot_noise) @ R
    t0 = t + rng.normal(size=3) * trans_noise
    prob = PoseProblem(_mat_to_quat(R0).astype(np.float32), t0.astype(np.float32), Xw.astype(np.float32),
                       uv.astype(np.float32), octave, inv_sigma2, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    return prob, dict(R=R, t=t, bad=bad)


def synthetic_projection_scene(n_kp=1000, n_mp=900, seed=5, dup_frac=0.15, distractor_frac=0.15,
                               claimed_frac=0.05, width=640, height=480, n_levels=8):
    """A tracked Frame plus MapPoints for the projection matchers.
    Keypoints uniform over the image (some on the far right / bottom edge, outside PosInGrid),
    random descriptors; MapPoints back-projected from keypoints at 1-8 m (pixel jitter ~ the
    keypoint scale, 0-40 flipped descriptor bits, rotation +12 deg), near-duplicates of the same
    keypoint (greedy conflicts) and random distractors. Returns a dict of arrays."""
    from ._lib import KP_DTYPE
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = D435I
    kps = np.zeros(n_kp, KP_DTYPE)
    kps["x"] = rng.uniform(0, width, n_kp).astype(np.float32)
    kps["y"] = rng.uniform(0, height, n_kp).astype(np.float32)
    edge = rng.random(n_kp) < 0.03
    kps["x"][edge] = rng.uniform(width - 6, width, edge.sum()).astype(np.float32)
    kps["octave"] = rng.integers(0, n_levels, n_kp)
    kps["angle"] = rng.uniform(0, 360, n_kp).astype(np.float32)
    kps["size"] = 31.0
    kps["response"] = rng.uniform(20, 80, n_kp).astype(np.float32)
    desc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    R = _rodrigues(rng.normal(size=3) * 0.4)
    t = rng.normal(size=3)
    q = _mat_to_quat(R).astype(np.float32)
    Rf = R.astype(np.float32)
    Ow = (-Rf.T @ t.astype(np.float32)).astype(np.float64)
    src = rng.choice(n_kp, n_mp, replace=False) if (dup_frac == 0 and n_mp <= n_kp) else \
        rng.integers(0, max(n_kp, 1), n_mp)
    ndup = int(dup_frac * n_mp)
    src[:ndup] = rng.integers(0, max(1, n_kp // 20), ndup)          # many points on few keypoints
    rng.shuffle(src)
    sc = np.power(1.2, kps["octave"][src])
    z = rng.uniform(1.0, 8.0, n_mp)
    u = kps["x"][src] + rng.normal(size=n_mp) * sc
    v = kps["y"][src] + rng.normal(size=n_mp) * sc
    Xc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1)
    pts = (Xc - t) @ R
    mdesc = desc[src].copy()
    for m in range(n_mp):
        nb = int(rng.integers(0, 41))
        bits = rng.choice(256, nb, replace=False)
        for b in bits:
            mdesc[m, b >> 3] ^= np.uint8(1 << (b & 7))
    dis = rng.random(n_mp) < distractor_frac
    mdesc[dis] = rng.integers(0, 256, (dis.sum(), 32), dtype=np.uint8)
    octave = np.clip(kps["octave"][src] + rng.integers(-1, 2, n_mp), 0, n_levels - 1).astype(np.int32)
    angle = ((kps["angle"][src] + 12.0 + rng.normal(size=n_mp) * 3.0) % 360.0).astype(np.float32)
    # MapPoint geometry for isInFrustum
    PO = pts - Ow
    dist = np.linalg.norm(PO, axis=1)
    normals = PO / dist[:, None] + rng.normal(size=(n_mp, 3)) * 0.05
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    back = rng.random(n_mp) < 0.05
    normals[back] *= -1
    max_dist = dist * rng.uniform(0.75, 1.4, n_mp)
    min_dist = max_dist / np.float64(1.2) ** (n_levels - 1)
    claimed = (rng.random(n_kp) < claimed_frac).astype(np.uint8)
    skip = (rng.random(n_mp) < 0.05).astype(np.uint8)
    return dict(kps=kps, desc=desc, pose_q=q, pose_t=t.astype(np.float32), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"],
                cy=cam["cy"], points=pts.astype(np.float32), mp_desc=mdesc, last_octave=octave, last_angle=angle,
                normals=normals.astype(np.float32), min_dist=min_dist.astype(np.float32),
                max_dist=max_dist.astype(np.float32), claimed=claimed, skip=skip, src=src)


def _flip_bits(rng, d, nb):
    d = d.copy()
    for b in rng.choice(256, nb, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def synthetic_init_pair(n1=1500, seed=9, width=640, height=480, n_levels=8, level0_frac=0.6, steal_frac=0.15,
                        distractor_frac=0.3, rot_deg=10.0, shift=(14.0, -6.0)):
    """Two frames for monocular initialisation (U:src/ORBmatcher.cc::SearchForInitialization):
    F1 keypoints (level0_frac on octave 0), F2 = F1 moved by `shift` px + jitter with 0-30
    flipped descriptor bits and a rotation of ~rot_deg (some random, for the histogram filter),
    some on octave 1 (level filter), plus distractors; `steal_frac` of the F1 level-0 keypoints get
    a later F1 twin near them whose descriptor is closer to the same F2 keypoint (the greedy
    steal path). F2 is shuffled. Returns (kps1, desc1, kps2, desc2, prev_matched)."""
    from ._lib import KP_DTYPE
    rng = np.random.Generator(np.random.PCG64(seed))
    k1 = np.zeros(n1, KP_DTYPE)
    k1["x"] = rng.uniform(0, width, n1).astype(np.float32)
    k1["y"] = rng.uniform(0, height, n1).astype(np.float32)
    k1["octave"] = np.where(rng.random(n1) < level0_frac, 0, rng.integers(1, n_levels, n1))
    k1["angle"] = rng.uniform(0, 360, n1).astype(np.float32)
    k1["size"] = 31.0
    k1["response"] = rng.uniform(20, 80, n1).astype(np.float32)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    k2, d2 = [], []
    for i in range(n1):
        if k1["octave"][i] != 0 or rng.random() < 0.2:
            continue
        r = np.zeros(1, KP_DTYPE)[0]
        r["x"] = np.float32(k1["x"][i] + shift[0] + rng.normal() * 3)
        r["y"] = np.float32(k1["y"][i] + shift[1] + rng.normal() * 3)
        r["octave"] = 0 if rng.random() > 0.05 else 1
        rot = rot_deg + rng.normal() * 2 if rng.random() > 0.1 else rng.uniform(0, 360)
        r["angle"] = np.float32((k1["angle"][i] - rot) % 360.0)
        r["size"] = 31.0
        r["response"] = np.float32(50)
        k2.append(r)
        d2.append(_flip_bits(rng, d1[i], int(rng.integers(0, 31))))
    # steals: a later F1 keypoint near i whose descriptor is closer to i's F2 partner
    n2m = len(k2)
    for j in rng.choice(n2m, int(steal_frac * n2m), replace=False):
        t = rng.integers(0, n1)
        k1["octave"][t] = 0
        k1["x"][t] = np.float32(k2[j]["x"] - shift[0] + rng.normal() * 5)
        k1["y"][t] = np.float32(k2[j]["y"] - shift[1] + rng.normal() * 5)
        k1["angle"][t] = np.float32((k2[j]["angle"] + rot_deg) % 360.0)
        d1[t] = _flip_bits(rng, d2[j], int(rng.integers(0, 12)))
    nd = int(distractor_frac * n2m)
    for _ in range(nd):
        r = np.zeros(1, KP_DTYPE)[0]
        r["x"] = np.float32(rng.uniform(0, width)); r["y"] = np.float32(rng.uniform(0, height))
        r["octave"] = 0; r["angle"] = np.float32(rng.uniform(0, 360)); r["size"] = 31.0; r["response"] = 40.0
        k2.append(r)
        # near-copies of a random F1 descriptor: second-best competition for the ratio test
        d2.append(_flip_bits(rng, d1[rng.integers(0, n1)], int(rng.integers(5, 40))))
    k2 = np.array(k2, KP_DTYPE)
    d2 = np.stack(d2).astype(np.uint8)
    perm = rng.permutation(k2.shape[0])
    k2, d2 = k2[perm], d2[perm]
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    return k1, d1, k2, d2, prev


def synthetic_kfdb_scene(n_kf=200, n_words=20000, words_per_place=400, seed=13, n_maps=2, common_pool=0,
                         common_frac=0.3):
    """A keyframe trajectory for KeyFrameDatabase queries. KF i sees the
    words of places i-2..i+2 (a sliding window, so neighbours share many words) plus random
    words; values positive, L1-normalised (DBoW2 BowVector). covis[i] = the 10 nearest KFs by
    index (GetBestCovisibilityKeyFrames order: most shared first), maps split the trajectory.
    A few KFs revisit an early place (loop closures). common_pool > 0 adds a pool of words every KF
    sees a fraction of (repetitive texture: many KFs pass the 0.8 x max common-words cut and the
    scores crowd). Returns dict(bows, covis, kf_map, place)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_places = n_kf + 4
    place_words = [rng.choice(n_words, words_per_place, replace=False) for _ in range(n_places)]
    place = np.arange(n_kf)
    loops = rng.choice(np.arange(n_kf // 2, n_kf), max(1, n_kf // 20), replace=False)
    place[loops] = rng.integers(0, n_kf // 4, loops.shape[0])
    pool = rng.choice(n_words, common_pool, replace=False) if common_pool else None
    bows = []
    for i in range(n_kf):
        ws = [] if pool is None else [pool[rng.random(common_pool) < common_frac]]
        for d in range(-2, 3):
            p = min(max(place[i] + d, 0), n_places - 1)
            pw = place_words[p]
            ws.append(pw[rng.random(pw.shape[0]) < 0.35])
        ws.append(rng.choice(n_words, 60, replace=False))
        w = np.unique(np.concatenate(ws)).astype(np.int32)
        v = rng.gamma(2.0, 1.0, w.shape[0])
        bows.append((w, v / v.sum()))
    covis = np.full((n_kf, 10), -1, np.int32)
    for i in range(n_kf):
        nb = sorted((j for j in range(max(0, i - 8), min(n_kf, i + 9)) if j != i), key=lambda j: (abs(i - j), j))
        covis[i, : min(10, len(nb))] = nb[:10]
    kf_map = (np.arange(n_kf) * n_maps // n_kf).astype(np.int32)
    return dict(bows=bows, covis=covis, kf_map=kf_map, place=place)


def synthetic_query_bow(scene, kf, seed, n_words=20000, keep=0.6, noise=80):
    """A frame near keyframe `kf` (or seeing several places: a list of KFs): a subset of their
    words plus noise words, L1-normalised."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kfs = [kf] if np.isscalar(kf) else list(kf)
    parts = []
    for k in kfs:
        w0, _ = scene["bows"][int(k)]
        parts.append(w0[rng.random(w0.shape[0]) < keep])
    w = np.unique(np.concatenate(parts + [rng.choice(n_words, noise, replace=False)])).astype(np.int32)
    v = rng.gamma(2.0, 1.0, w.shape[0])
    return w, v / v.sum()


def banded_pose_system(n_pose, w, cyclic, seed, n_land=None):
    """A reduced-camera-system-shaped SPD matrix: S = sum of landmark terms v v^T, each over the
    6-vectors of a window of <= w + 1 consecutive poses (cyclic: windows wrap around, a keyframe
    loop), + 0.5 I; and the pose blocks (i <= j) of its structure. (399 poses, w = 19, cyclic: the
    C5 GBA's system) Returns (S, b, block_i, block_j)."""
    rng = np.random.default_rng(seed)
    n = 6 * n_pose
    A = np.zeros((n, n))
    blocks = set()
    for _ in range(n_land or 6 * n_pose):
        s = int(rng.integers(0, n_pose if cyclic else n_pose - w))
        ln = int(rng.integers(2, w + 2))
        poses = [(s + k) % n_pose for k in range(ln) if cyclic or s + k < n_pose]
        idx = np.concatenate([np.arange(6 * p, 6 * p + 6) for p in poses])
        v = rng.normal(size=idx.size)
        A[np.ix_(idx, idx)] += np.outer(v, v)
        for a in poses:
            for b in poses:
                blocks.add((min(a, b), max(a, b)))
    for p in range(n_pose):
        blocks.add((p, p))
    A += np.eye(n) * 0.5
    bi = np.array([b[0] for b in sorted(blocks)], np.int32)
    bj = np.array([b[1] for b in sorted(blocks)], np.int32)
    return A, rng.normal(size=n), bi, bj


# ---------------------------------------------------------------------------
# SearchForTriangulation scenes (LocalMapping::CreateNewMapPoints)
# ---------------------------------------------------------------------------
def orb_scale_tables(n_levels=8, scale_factor=1.2):
    """(mvScaleFactors, mvLevelSigma2) as the ORBextractor ctor fills them (float32)."""
    sf = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sf[i] = np.float32(np.float64(sf[i - 1]) * np.float64(np.float32(scale_factor)))
    return sf, (sf * sf).astype(np.float32)


def quat_to_rot64(q):
    """The rotation a float32 quaternion (x, y, z, w) stands for, in float64."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pinhole_project(q, t, cam, P):
    """World points P (m, 3) through Tcw = (q, t) and the pinhole cam: (uv (m, 2), depth (m,)), float64."""
    Xc = P @ quat_to_rot64(q).T + np.asarray(t, np.float64)
    z = Xc[:, 2]
    uv = np.stack([cam["fx"] * Xc[:, 0] / z + cam["cx"], cam["fy"] * Xc[:, 1] / z + cam["cy"]], 1)
    return uv, z


def synthetic_triangulation_scene(n=300, B=3, seed=0, n_nodes=12, n2=None, mp_frac=1.0 / 3, n_levels=8,
                                  scale_factor=1.2, cam=None):
    """A keyframe with n features and B covisible neighbours that see common 3-D points, for
    SearchForTriangulation. Neighbour b moves sideways (b % 3 == 0), forward along the optical axis
    (b % 3 == 1: its epipole lies inside the image) or diagonally (b % 3 == 2), each with a small
    rotation. KF1's features are the noise-free projections of points 2-8 m away; a neighbour sees
    90 % of them (the "twins") with pixel noise of half a level sigma (15 % displaced by 2.5-8 sigma:
    epipolar outliers), 0-30 flipped descriptor bits, the keyframe's in-plane rotation (12 % random:
    the orientation filter), node ids from an alphabet of n_nodes (7 % moved to another node), some
    weights 0 and nodes -1; mp_frac of KF1's features carry MapPoints (their twins mostly too), plus
    random distractors. Planted: on every forward neighbour, twins within 6 px of the epipole (the
    epipole exclusion); exact copies of twins (equal distances: the later index wins); KF1 features
    duplicated next to themselves (two KF1 features share one target). Each neighbour is shuffled.
    n2: features per neighbour (an int, or one per neighbour): twins are dropped / distractors added
    to reach it. Returns a dict: kf1, neighbours (TriKeyFrame), scale_factors, level_sigma2, twin[b]
    (n,) = the neighbour feature that is KF1 feature i's twin or -1, epi[b] = KF1 features planted at
    neighbour b's epipole."""
    from ._lib import KP_DTYPE
    from .matcher import TriKeyFrame
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = dict(D435I if cam is None else cam)
    W, H = cam["w"], cam["h"]
    sf, s2 = orb_scale_tables(n_levels, scale_factor)
    alphabet = np.sort(rng.choice(np.arange(1000, 1_000_000), n_nodes, replace=False)).astype(np.int32)
    R1 = _rodrigues(rng.normal(size=3) * 0.05)
    t1 = rng.normal(size=3) * 0.1
    q1 = _mat_to_quat(R1).astype(np.float32)
    t1 = t1.astype(np.float32)
    R1 = quat_to_rot64(q1)
    # neighbour poses, relative to KF1's camera frame: X2 = Rrel (X1 - c)
    poses, rels = [], []
    for b in range(B):
        kind = b % 3
        c = (np.array([0.35, 0.02, 0.0]), np.array([0.01, -0.01, 0.45]), np.array([-0.25, 0.15, 0.05]))[kind].copy()
        if b >= 3:
            c *= rng.uniform(0.6, 1.5)
            c[:2] += rng.normal(size=2) * (0.005 if kind == 1 else 0.05)
        Rrel = _rodrigues(rng.normal(size=3) * 0.03)
        q2 = _mat_to_quat(Rrel @ R1).astype(np.float32)
        t2 = (Rrel @ (t1.astype(np.float64) - c)).astype(np.float32)
        poses.append((q2, t2))
        rels.append((Rrel, c))
    fwd = [b for b in range(B) if b % 3 == 1]
    n_epi = min(8, n // 20) if fwd else 0
    n_dup = n // 40
    if n_epi * len(fwd) + n_dup > n // 2:      # a small keyframe against many neighbours: no plants
        n_epi = n_dup = 0
    n_pts = n - n_epi * len(fwd) - n_dup
    # 3-D points in KF1's camera frame
    u = rng.uniform(20, W - 20, n_pts); v = rng.uniform(20, H - 20, n_pts); z = rng.uniform(2.0, 8.0, n_pts)
    X1 = [np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1)]
    epi_of = np.full(n, -1, np.int64)   # KF1 feature -> the neighbour whose epipole it was planted at
    pos = n_pts
    for b in fwd:
        Rrel, c = rels[b]
        e2 = Rrel @ (-c)                                           # KF1's centre in KF2's frame
        ep = np.array([cam["fx"] * e2[0] / e2[2] + cam["cx"], cam["fy"] * e2[1] / e2[2] + cam["cy"]])
        ang = rng.uniform(0, 2 * np.pi, n_epi); rad = rng.uniform(0.5, 6.0, n_epi); d = rng.uniform(3.0, 8.0, n_epi)
        px = ep[0] + rad * np.cos(ang); py = ep[1] + rad * np.sin(ang)
        X2 = np.stack([(px - cam["cx"]) / cam["fx"] * d, (py - cam["cy"]) / cam["fy"] * d, d], 1)
        X1.append(X2 @ Rrel + c)                                   # X1 = Rrel^T X2 + c
        epi_of[pos:pos + n_epi] = b
        pos += n_epi
    X1 = np.concatenate(X1)
    Pw = (X1 - t1.astype(np.float64)) @ R1                         # Xw = R1^T (X1 - t1)
    n_real = X1.shape[0]
    # KF1 features: one per point, then duplicates of unclaimed features next to themselves
    k1 = np.zeros(n, KP_DTYPE)
    uv1, _ = pinhole_project(q1, t1, cam, Pw)
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    node1 = alphabet[rng.integers(0, n_nodes, n)]
    w1 = rng.uniform(0.1, 1.0, n)
    mp1 = (rng.random(n) < mp_frac).astype(np.uint8)
    k1["x"][:n_real] = uv1[:, 0].astype(np.float32); k1["y"][:n_real] = uv1[:, 1].astype(np.float32)
    k1["octave"] = np.minimum(rng.integers(0, n_levels, n), rng.integers(0, n_levels, n))
    k1["angle"] = rng.integers(0, 360, n).astype(np.float32)
    k1["size"] = 31.0
    k1["response"] = rng.uniform(20, 80, n).astype(np.float32)
    planted = epi_of >= 0
    if mp_frac < 1.0:
        mp1[planted] = 0
    src_of = np.arange(n)                                          # the point feature a duplicate copies
    for j in range(n_real, n):
        i = int(rng.integers(0, n_pts))
        src_of[j] = i
        if mp_frac < 1.0:
            mp1[i] = mp1[j] = 0
        k1["x"][j] = np.float32(k1["x"][i] + rng.uniform(-0.3, 0.3)); k1["y"][j] = np.float32(k1["y"][i] + rng.uniform(-0.3, 0.3))
        k1["angle"][j] = k1["angle"][i]
        d1[j] = _flip_bits(rng, d1[i], int(rng.integers(1, 7)))
        node1[j] = node1[i]
    bad = rng.random(n)
    free = ~planted & (src_of == np.arange(n)) & ~np.isin(np.arange(n), src_of[n_real:])
    w1[free & (bad < 0.03)] = 0.0
    node1[free & (bad > 0.98)] = -1
    kf1 = TriKeyFrame(k1, d1, node1, w1, mp1, q1, t1, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    n2 = [n2] * B if n2 is None or np.isscalar(n2) else list(n2)
    neighbours, twins = [], []
    for b in range(B):
        q2, t2 = poses[b]
        uv2, z2 = pinhole_project(q2, t2, cam, Pw)
        rot_b = 7.0 + 11.0 * (b % 7)
        rows = []                                                  # (kp fields, desc, node, weight, mp, twin of)
        def feat(x, y, octave, angle, desc, node, weight, mp, of):
            r = np.zeros(1, KP_DTYPE)[0]
            a = np.float32(angle % 360.0)
            r["x"], r["y"], r["octave"], r["angle"] = np.float32(x), np.float32(y), octave, (a if a < 360 else 0.0)
            r["size"], r["response"] = 31.0, 50.0
            rows.append((r, desc, node, weight, mp, of))
        tie_left = max(3, n // 60)
        for i in range(n_real):
            at_epi = epi_of[i] == b
            inside = z2[i] > 0.1 and 0 <= uv2[i, 0] < W and 0 <= uv2[i, 1] < H
            if not inside or (not at_epi and rng.random() > 0.9):
                continue
            octave = int(min(rng.integers(0, n_levels), rng.integers(0, n_levels)))
            sig = float(sf[octave])
            if at_epi:
                octave, sig = int(rng.integers(0, 3)), 0.0
                dx, dy = rng.normal(size=2) * 0.2
            elif rng.random() < 0.15:
                a = rng.uniform(0, 2 * np.pi); r_ = rng.uniform(2.5, 8.0) * sig
                dx, dy = r_ * np.cos(a), r_ * np.sin(a)
            else:
                dx, dy = rng.normal(size=2) * 0.5 * sig
            angle = k1["angle"][i] - rot_b + rng.normal() * 2.0 if (at_epi or rng.random() > 0.12) else rng.uniform(0, 360)
            node = node1[i]
            if not at_epi and rng.random() < 0.07:
                node = alphabet[rng.integers(0, n_nodes)]
            weight = 0.0 if (not at_epi and rng.random() < 0.03) else rng.uniform(0.1, 1.0)
            if not at_epi and rng.random() < 0.02:
                node = -1
            mp = 0 if at_epi else int(rng.random() < (0.85 if mp1[i] else 0.05))
            desc = _flip_bits(rng, d1[i], int(rng.integers(0, 11 if at_epi else 31)))
            feat(uv2[i, 0] + dx, uv2[i, 1] + dy, octave, angle, desc, node, weight, mp, i)
            if tie_left and not at_epi and not mp and not mp1[i] and node == node1[i] and weight > 0 and w1[i] > 0 \
                    and node >= 0 and abs(dx) + abs(dy) < sig:
                tie_left -= 1                                      # an exact copy: equal distance, the later index wins
                feat(uv2[i, 0] + dx, uv2[i, 1] + dy, octave, angle, desc.copy(), node, weight, 0, -1)
        target = n2[b]
        n_dis = int(0.2 * n) if target is None else max(target - len(rows), 0)
        if target is not None and len(rows) > target:
            keep = np.sort(rng.permutation(len(rows))[:target])
            rows = [rows[k] for k in keep]
        for _ in range(n_dis):
            feat(rng.uniform(0, W), rng.uniform(0, H), int(rng.integers(0, n_levels)), rng.uniform(0, 360),
                 rng.integers(0, 256, 32, dtype=np.uint8), alphabet[rng.integers(0, n_nodes)], rng.uniform(0.1, 1.0),
                 int(rng.random() < 0.1), -1)
        perm = rng.permutation(len(rows))
        rows = [rows[k] for k in perm]
        m = len(rows)
        k2 = np.array([r[0] for r in rows], KP_DTYPE) if m else np.zeros(0, KP_DTYPE)
        d2 = np.stack([r[1] for r in rows]).astype(np.uint8) if m else np.zeros((0, 32), np.uint8)
        twin = np.full(n, -1, np.int64)
        for j, r in enumerate(rows):
            if r[5] >= 0:
                twin[r[5]] = j
        neighbours.append(TriKeyFrame(k2, d2, np.array([r[2] for r in rows], np.int32),
                                      np.array([r[3] for r in rows], np.float64),
                                      np.array([r[4] for r in rows], np.uint8), q2, t2, cam["fx"], cam["fy"],
                                      cam["cx"], cam["cy"]))
        twins.append(twin)
    return dict(kf1=kf1, neighbours=neighbours, scale_factors=sf, level_sigma2=s2, twin=twins,
                epi=[np.nonzero(epi_of == b)[0] for b in range(B)], cam=cam)


# ---------------------------------------------------------------------------
# CreateNewMapPoints scenes: the triangulation and its checks on the matches above
# ---------------------------------------------------------------------------
WIDE_CAM = dict(fx=300.0, fy=300.0, cx=320.0, cy=240.0, w=640, h=480)   # 94 x 77 degrees: rays may be > 90 degrees apart
NEW_POINT_KINDS = ("far", "behind", "between", "apart", "reproj1", "reproj2", "octave")


def _pose64(k):
    return quat_to_rot64(k.pose_q), np.asarray(k.pose_t, np.float64)


def new_point_status64(k1, k2, p1, p2, o1, o2, sf, s2, cos_max=0.9998, ratio_factor=None, far=0.0):
    """The status CreateNewMapPoints gives a pair of pixels, in float64 with numpy's SVD (the
    library's rule is DESIGN.md's fp32 / Jacobi restatement: the two agree away from the gates). The
    generator places its plants with this."""
    ratio_factor = 1.5 * float(sf[1]) if ratio_factor is None else ratio_factor
    rays, rows, cams = [], [], []
    for k, p in ((k1, p1), (k2, p2)):
        R, t = _pose64(k)
        xn = np.array([(p[0] - k.cx) / k.fx, (p[1] - k.cy) / k.fy, 1.0])
        rays.append(R.T @ xn)
        T = np.concatenate([R, t[:, None]], 1)
        rows += [xn[0] * T[2] - T[0], xn[1] * T[2] - T[1]]
        cams.append((R, t, k))
    cosP = rays[0] @ rays[1] / (np.linalg.norm(rays[0]) * np.linalg.norm(rays[1]))
    if not cosP > 0:
        return 2
    if not cosP < cos_max:
        return 3
    v = np.linalg.svd(np.array(rows))[2][3]
    if v[3] == 0:
        return 4
    X = v[:3] / v[3]
    zs = [(R @ X + t)[2] for R, t, _ in cams]
    if zs[0] <= 0:
        return 5
    if zs[1] <= 0:
        return 6
    dist = []
    for code, (R, t, k), p, o in ((7, cams[0], p1, o1), (8, cams[1], p2, o2)):
        Xc = R @ X + t
        e = np.array([k.fx * Xc[0] / Xc[2] + k.cx - p[0], k.fy * Xc[1] / Xc[2] + k.cy - p[1]])
        if e @ e > 5.991 * float(s2[o]):
            return code
        dist.append(np.linalg.norm(X + R.T @ t))
    if dist[0] == 0 or dist[1] == 0:
        return 9
    if far > 0 and (dist[0] >= far or dist[1] >= far):
        return 10
    rd, ro = dist[1] / dist[0], float(sf[o1]) / float(sf[o2])
    return 11 if (rd * ratio_factor < ro or rd > ro * ratio_factor) else 1


def synthetic_new_points_scene(n=300, B=3, seed=0, cam=None, n_plant=4, far_threshold=7.0, median_depth=4.0,
                               gated_at=1, scale=0.02, **scene_args):
    """synthetic_triangulation_scene(n, B, seed, cam=WIDE_CAM by default) prepared for
    CreateNewMapPoints. Per neighbour and kind, up to n_plant of its matched twins are rewritten
    (descriptor within 3 bits of the KF1 feature's, same node, no MapPoint, consistent angle, so the
    search takes them) into
      far      the projection of the KF1 ray's point at 500 m (parallax too low),
      behind   ... at a negative depth (the rays diverge: not in front of KF1),
      between  ... between the two camera centres of a forward neighbour (behind KF2),
      apart    ... the same with a KF1 feature moved towards a corner: the rays are > 90 degrees apart,
      reproj1  an octave-0 KF1 feature, the twin at octave 6 and 1.8 of its sigmas off the epipolar
               line: inside the search's gate, its half across the 5.991 gate of image 1 only,
      reproj2  on a forward neighbour, a KF1 feature at octave 7 whose point lies 6-25 m away
               (parallax just inside the gate), the twin at octave 7 and 1.5-1.9 of its sigmas off the
               epipolar line: see scale,
      octave   octaves 3 apart against the change of distance of a forward neighbour, or 5 apart.
    scale: the length of the base scene's metre in map units (every translation, far_threshold and
    median_depth are multiplied by it; the images do not change). A monocular map has an arbitrary
    unit, and the null vector of the 4x4 system is not invariant to it: the vector is normalised
    with its fourth component, so where coordinates are small against 1 the residual of an image
    weighs with the point's depth in it, and at low parallax the solution slides along KF1's ray
    towards KF2 until image 2 alone fails its 5.991 gate, although the twin lies inside the 3.84 gate
    of the search (reproj2; in metres, scale = 1, no searched pair does). far_threshold cuts the
    points beyond it; a neighbour 1 mm from KF1 (a copy of the first, gated against median_depth,
    the scene depth given for every neighbour) is inserted at index gated_at (None: not). Returns the base scene's dict with neighbours and median_depth including the gated
    neighbour, far_threshold, gated (B,), plants = [(kind, neighbour, idx1, idx2)]."""
    from .matcher import TriKeyFrame
    cam = dict(WIDE_CAM if cam is None else cam)
    s = synthetic_triangulation_scene(n, B, seed, cam=cam, **scene_args)
    m = float(scale)                                               # one metre of the base scene
    for k in [s["kf1"]] + s["neighbours"]:
        k.pose_t = (k.pose_t.astype(np.float64) * m).astype(np.float32)
    far_threshold, median_depth = far_threshold * m, median_depth * m
    rng = np.random.Generator(np.random.PCG64(1000003 * (seed + 1)))
    k1, sf, s2 = s["kf1"], s["scale_factors"], s["level_sigma2"]
    W, H = cam["w"], cam["h"]
    R1, t1 = _pose64(k1)
    used = set(int(i) for e in s["epi"] for i in e)
    plants = []

    def world(p1, lam):   # the point of depth lam on KF1's ray through pixel p1
        X1 = lam * np.array([(p1[0] - cam["cx"]) / cam["fx"], (p1[1] - cam["cy"]) / cam["fy"], 1.0])
        return (X1 - t1) @ R1

    def project(k, Xw):
        R, t = _pose64(k)
        Xc = R @ Xw + t
        return np.array([cam["fx"] * Xc[0] / Xc[2] + cam["cx"], cam["fy"] * Xc[1] / Xc[2] + cam["cy"]])

    for b, k2 in enumerate(s["neighbours"]):
        twin = s["twin"][b]
        forward = b % 3 == 1
        e1 = project(k1, -_pose64(k2)[0].T @ _pose64(k2)[1])      # KF2's centre in image 1
        e2 = project(k2, -R1.T @ t1)                              # KF1's centre in image 2
        free = [int(i) for i in rng.permutation(n) if twin[i] >= 0 and not k1.has_mp[i] and k1.node[i] >= 0
                and k1.weight[i] > 0 and int(i) not in used]
        rot_b = 7.0 + 11.0 * (b % 7)
        for kind in NEW_POINT_KINDS:
            want = dict(far=3, behind=5, between=6, apart=2, reproj1=7, reproj2=8, octave=11)[kind]
            if (kind in ("between", "apart", "reproj2") and not forward) or (kind == "behind" and forward):
                continue
            done = tries = 0
            for _ in range(400 * n_plant):
                if done == n_plant or not free:
                    break
                i = free[0]
                j = int(twin[i])
                p1 = np.array([k1.kps["x"][i], k1.kps["y"][i]], np.float64)
                o1 = int(k1.kps["octave"][i])
                o2 = int(k2.kps["octave"][j])
                if kind == "far":
                    p2 = project(k2, world(p1, 500.0 * m))
                elif kind == "behind":
                    p2 = project(k2, world(p1, -rng.uniform(2.0, 8.0) * m))
                elif kind == "between":
                    p2 = project(k2, world(p1, rng.uniform(0.1, 0.35) * m))
                elif kind == "apart":
                    p1 = np.array([rng.choice([25.0, W - 25.0]), rng.choice([25.0, H - 25.0])]) + rng.uniform(-5, 5, 2)
                    p2 = project(k2, world(p1, rng.uniform(0.2, 0.225) * m))
                elif kind == "reproj1":
                    o1, o2 = 0, 6
                    z = rng.uniform(2.0, 8.0) * m
                    a, c = project(k2, world(p1, z)), project(k2, world(p1, z + 0.5 * m))
                    nrm = np.array([-(c - a)[1], (c - a)[0]]) / np.linalg.norm(c - a)
                    p2 = a + rng.choice([-1.0, 1.0]) * 1.8 * float(sf[o2]) * nrm
                elif kind == "reproj2":
                    o1 = o2 = 7
                    p1 = np.array([rng.uniform(5.0, W - 5.0), rng.uniform(5.0, H - 5.0)])
                    z = rng.uniform(6.0, 25.0) * m
                    a, c = project(k2, world(p1, z)), project(k2, world(p1, 1.05 * z))
                    nrm = np.array([-(c - a)[1], (c - a)[0]]) / np.linalg.norm(c - a)
                    p2 = a + rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 1.9) * float(sf[o2]) * nrm
                else:
                    if forward:
                        o2 = int(rng.integers(0, 5)); o1 = o2 + 3
                    else:
                        o1, o2 = (0, 5) if rng.random() < 0.5 else (5, 0)
                    p2 = project(k2, world(p1, rng.uniform(2.0, 5.5) * m))
                p1 = p1.astype(np.float32).astype(np.float64)
                p2 = p2.astype(np.float32).astype(np.float64)
                inside = all(1 <= p[0] < W - 1 and 1 <= p[1] < H - 1 for p in (p1, p2))
                clear = np.linalg.norm(p2 - e2) > 12.0 * np.sqrt(float(sf[o2]))
                if not (inside and clear and new_point_status64(k1, k2, p1, p2, o1, o2, sf, s2,
                                                                far=far_threshold) == want):
                    tries += 1
                    if tries >= (60 if kind in ("between", "apart") else 400 if kind == "reproj2" else 1):   # the next feature
                        free.pop(0)
                        tries = 0
                    continue
                free.pop(0)
                tries = 0
                used.add(i)
                k1.kps["x"][i], k1.kps["y"][i], k1.kps["octave"][i] = p1[0], p1[1], o1
                k2.kps["x"][j], k2.kps["y"][j], k2.kps["octave"][j] = p2[0], p2[1], o2
                k2.kps["angle"][j] = np.float32((float(k1.kps["angle"][i]) - rot_b) % 360.0) % np.float32(360.0)
                k2.desc[j] = _flip_bits(rng, k1.desc[i], int(rng.integers(0, 4)))
                k2.node[j], k2.weight[j], k2.has_mp[j] = k1.node[i], 0.5, 0
                plants.append((kind, b, i, j))
                done += 1
    nbrs, md = list(s["neighbours"]), [float(median_depth)] * B
    gated = np.zeros(B, np.uint8)
    if gated_at is not None and B > 0:
        g0 = nbrs[0]
        t2 = (np.asarray(k1.pose_t, np.float64) - np.array([0.001 * m, 0.0, 0.0])).astype(np.float32)
        near = TriKeyFrame(g0.kps.copy(), g0.desc.copy(), g0.node.copy(), g0.weight.copy(), g0.has_mp.copy(),
                           k1.pose_q.copy(), t2, k1.fx, k1.fy, k1.cx, k1.cy)
        nbrs.insert(gated_at, near)
        md.insert(gated_at, float(median_depth))
        gated = np.insert(gated, gated_at, 1).astype(np.uint8)
        plants = [(kind, b + (b >= gated_at), i, j) for kind, b, i, j in plants]
    s.update(neighbours=nbrs, median_depth=np.array(md, np.float32), far_threshold=float(far_threshold), gated=gated,
             plants=plants)
    s["twin"] = None   # the base scene's twin table does not describe the rewritten neighbours
    return s


# ---------------------------------------------------------------------------
# Fuse scenes (LocalMapping::SearchInNeighbors)
# ---------------------------------------------------------------------------
FUSE_KINDS = ("plain", "th_low", "chi2", "level", "twin_same", "twin_cell", "none", "behind", "outside", "far",
              "near", "angle")


def fuse_level_margin(kfs, points, max_dist):
    """min over the keyframes of |x - nearest integer|, x = log(max_dist / dist3D) / log_scale_factor
    in float64 from the float32 inputs, per MapPoint: how far PredictScale's ceil is from a step."""
    P = np.asarray(points, np.float64)
    out = np.full(P.shape[0], np.inf)
    for k in kfs:
        R = quat_to_rot64(k.pose_q)
        Ow = -R.T @ np.asarray(k.pose_t, np.float64)
        d = np.linalg.norm(P - Ow, axis=1)
        with np.errstate(all="ignore"):
            x = np.log(np.asarray(max_dist, np.float64) / d) / float(k.log_scale_factor)
        out = np.minimum(out, np.abs(x - np.rint(x)))
    return out


def synthetic_fuse_scene(n_kp=300, n_mp=300, B=3, seed=0, n_levels=8, scale_factor=1.2, th=3.0, cam=None,
                         radius=4.5, arc=0.7):
    """B keyframes on an arc of `arc` radians, `radius` m from one cloud of n_mp MapPoints they all
    look at, for ORBmatcher.Fuse. n_kp: keypoints per keyframe (an int, or one per keyframe). Every
    point has a kind (FUSE_KINDS, returned as `kind`) that says what each keyframe that sees it gets:
      plain      one keypoint within 1.5 level sigma of the projection, octave = the predicted level or
                 one below, 0-40 descriptor bits flipped
      th_low     as plain with 49 / 50 / 51 / 52 flipped bits (both sides of TH_LOW)
      chi2       one keypoint 2.44 or 2.455 level sigma away (5.99 = 2.4474^2: inside / outside)
      level      an exact copy of the descriptor at octave level - 2 or level + 1 (outside the gate),
                 and mostly a proper keypoint with 20 flipped bits
      twin_same  a plain keypoint and an equal copy 0.25 px beside it (usually the same cell)
      twin_cell  two equal copies 3.2 level sigma apart in x (levels >= 5: usually different cells)
      none       no keypoint
      behind / outside / far / near / angle   the point lies behind the cameras / outside the images /
                 beyond 1.2 mfMaxDistance / below 0.8 mfMinDistance / is seen at more than 60 degrees
    The distance ranges put the predicted levels across 0 .. n_levels - 1. A point whose
    log(max_dist / dist3D) / log_scale_factor comes within 2e-3 of an integer for some keyframe gets
    its distance range scaled by 1.01 until none does (fuse_level_margin), so a last-bit difference
    between two logf implementations cannot move a level. Keypoints are shuffled; a keyframe with
    fewer planted keypoints than n_kp is filled with random ones, one with more drops the excess.
    Returns a dict: kfs (ProjFrame), points, normals, min_dist, max_dist, mp_desc, skip, pair_skip,
    scale_factors, inv_level_sigma2, th, kind, nudged (how many points had their range scaled)."""
    from ._lib import KP_DTYPE
    from .matcher import ProjFrame
    rng = np.random.Generator(np.random.PCG64(seed))
    cam = dict(D435I if cam is None else cam)
    W, H = cam["w"], cam["h"]
    sf, s2 = orb_scale_tables(n_levels, scale_factor)
    inv_s2 = (np.float32(1.0) / s2).astype(np.float32)
    n_kps = [int(n_kp)] * B if np.isscalar(n_kp) else [int(v) for v in n_kp]
    assert len(n_kps) == B
    # the keyframes
    thetas = np.linspace(-arc / 2, arc / 2, B) if B > 1 else np.zeros(1)
    poses, centres = [], []
    for b in range(B):
        c = radius * np.array([np.sin(thetas[b]), 0.1 * np.sin(3 * thetas[b]), -np.cos(thetas[b])])
        R = _rodrigues(rng.normal(size=3) * 0.02) @ _look_at(c)
        q = _mat_to_quat(R).astype(np.float32)
        t = (-(quat_to_rot64(q) @ c)).astype(np.float32)
        poses.append((q, t))
        centres.append(-quat_to_rot64(q).T @ t.astype(np.float64))
    mid = np.mean(centres, axis=0) if B else np.array([0.0, 0.0, -radius])
    # the points
    kind = rng.choice(len(FUSE_KINDS), n_mp, p=[0.44, 0.07, 0.07, 0.06, 0.06, 0.06, 0.06, 0.03, 0.04, 0.04, 0.03,
                                               0.04])
    K = {name: i for i, name in enumerate(FUSE_KINDS)}
    P = np.stack([rng.uniform(-1.8, 1.8, n_mp), rng.uniform(-1.3, 1.3, n_mp), rng.uniform(-0.6, 0.6, n_mp)], 1)
    P[kind == K["behind"]] = mid * rng.uniform(1.3, 2.0, (int((kind == K["behind"]).sum()), 1)) + \
        rng.normal(size=(int((kind == K["behind"]).sum()), 3)) * 0.3
    side = kind == K["outside"]
    P[side, 0] = rng.choice([-1.0, 1.0], int(side.sum())) * rng.uniform(5.0, 8.0, int(side.sum()))
    P = P.astype(np.float32)
    P64 = P.astype(np.float64)
    PO = P64 - mid
    d_ref = np.linalg.norm(PO, axis=1)
    normals = PO / d_ref[:, None] + rng.normal(size=(n_mp, 3)) * 0.03
    ang = kind == K["angle"]
    if ang.any():   # tilt by 70-85 degrees about an axis perpendicular to the viewing ray
        for m in np.nonzero(ang)[0]:
            axis = np.cross(PO[m], rng.normal(size=3))
            axis /= np.linalg.norm(axis)
            normals[m] = _rodrigues(axis * np.deg2rad(rng.uniform(70, 85))) @ (PO[m] / d_ref[m])
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    target = rng.integers(0, n_levels, n_mp)
    twin_cell = kind == K["twin_cell"]
    target[twin_cell] = rng.integers(min(5, n_levels - 1), n_levels, int(twin_cell.sum()))
    max_dist = d_ref * np.float64(scale_factor) ** (target - 0.5)
    max_dist[kind == K["far"]] = d_ref[kind == K["far"]] * rng.uniform(0.5, 0.75, int((kind == K["far"]).sum()))
    near = kind == K["near"]
    max_dist[near] = d_ref[near] * rng.uniform(1.4, 1.8, int(near.sum())) * np.float64(scale_factor) ** (n_levels - 1)
    max_dist = max_dist.astype(np.float32)
    probe = [ProjFrame(np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), q, t, cam["fx"], cam["fy"], cam["cx"],
                       cam["cy"], W, H, scale_factor, n_levels) for q, t in poses]
    nudged = np.zeros(n_mp, bool)
    for _ in range(200):
        close = fuse_level_margin(probe, P, max_dist) <= 2e-3
        if not close.any():
            break
        nudged |= close
        max_dist[close] = (max_dist[close] * np.float32(1.01)).astype(np.float32)
    else:
        raise RuntimeError("synthetic_fuse_scene: the level margin could not be reached")
    min_dist = (max_dist.astype(np.float64) / np.float64(scale_factor) ** (n_levels - 1)).astype(np.float32)
    mp_desc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    log_sf = float(probe[0].log_scale_factor) if B else float(np.log(np.float32(scale_factor)))
    # the keypoints of every keyframe
    kfs = []
    for b in range(B):
        q, t = poses[b]
        uv, z = pinhole_project(q, t, cam, P64)
        dist = np.linalg.norm(P64 - centres[b], axis=1)
        with np.errstate(all="ignore"):
            lvl = np.clip(np.ceil(np.log(max_dist.astype(np.float64) / dist) / log_sf), 0, n_levels - 1).astype(int)
        seen = (z > 0.1) & (uv[:, 0] > 8) & (uv[:, 0] < W - 8) & (uv[:, 1] > 8) & (uv[:, 1] < H - 8)
        rows = []   # (x, y, octave, descriptor)

        def plant(m, rho, octave, desc, direction=None):
            a = rng.uniform(0, 2 * np.pi) if direction is None else direction
            e = rho * float(sf[octave])
            rows.append((uv[m, 0] + e * np.cos(a), uv[m, 1] + e * np.sin(a), octave, desc))

        for m in np.nonzero(seen)[0]:
            L = int(lvl[m])
            below = L - 1 if (L > 0 and rng.random() < 0.3) else L
            kd = FUSE_KINDS[kind[m]]
            if kd == "plain":
                plant(m, rng.uniform(0, 1.5), below, _flip_bits(rng, mp_desc[m], int(rng.integers(0, 41))))
            elif kd == "th_low":
                plant(m, rng.uniform(0, 1.5), below, _flip_bits(rng, mp_desc[m], int(rng.choice([49, 50, 51, 52]))))
            elif kd == "chi2":
                plant(m, float(rng.choice([2.44, 2.455])), L, _flip_bits(rng, mp_desc[m], 10))
            elif kd == "level":
                wrong = L - 2 if L >= 2 else L + 1
                if 0 <= wrong < n_levels:
                    plant(m, rng.uniform(0, 0.3), wrong, mp_desc[m].copy())
                if rng.random() < 0.6:
                    plant(m, rng.uniform(0, 1.5), below, _flip_bits(rng, mp_desc[m], 20))
            elif kd == "twin_same" or (kd == "twin_cell" and L < 5):
                d = _flip_bits(rng, mp_desc[m], int(rng.integers(0, 31)))
                plant(m, rng.uniform(0, 1.0), below, d)
                x, y, o, _ = rows[-1]
                rows.append((x + 0.25, y, o, d.copy()))
            elif kd == "twin_cell":
                d = _flip_bits(rng, mp_desc[m], int(rng.integers(0, 31)))
                plant(m, 1.6, L, d, direction=0.0)
                plant(m, 1.6, L, d.copy(), direction=np.pi)
        nb = n_kps[b]
        order = rng.permutation(len(rows))[:nb]
        kps = np.zeros(nb, KP_DTYPE)
        desc = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
        kps["x"] = rng.uniform(0, W, nb).astype(np.float32)
        kps["y"] = rng.uniform(0, H, nb).astype(np.float32)
        kps["octave"] = rng.integers(0, n_levels, nb)
        for slot, r in enumerate(order):
            x, y, o, d = rows[r]
            kps["x"][slot], kps["y"][slot], kps["octave"][slot] = np.float32(x), np.float32(y), o
            desc[slot] = d
        shuffle = rng.permutation(nb)
        kps, desc = kps[shuffle], desc[shuffle]
        kps["angle"] = rng.uniform(0, 360, nb).astype(np.float32)
        kps["size"] = (31.0 * sf[kps["octave"]]).astype(np.float32)
        kps["response"] = rng.uniform(20, 80, nb).astype(np.float32)
        kfs.append(ProjFrame(kps, desc, q, t, cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H, scale_factor,
                             n_levels))
    skip = (rng.random(n_mp) < 0.03).astype(np.uint8)
    pair_skip = (rng.random((B, n_mp)) < 0.03).astype(np.uint8)
    return dict(kfs=kfs, points=P, normals=normals.astype(np.float32), min_dist=min_dist, max_dist=max_dist,
                mp_desc=mp_desc, skip=skip, pair_skip=pair_skip, scale_factors=sf, inv_level_sigma2=inv_s2,
                th=float(th), kind=np.array(FUSE_KINDS)[kind], nudged=int(nudged.sum()))


# ---------------------------------------------------------------------------
# Sim3 scenes (LoopClosing: SearchByProjection with a Sim3)
# ---------------------------------------------------------------------------
def synthetic_sim3_scene(n_kp=300, n_mp=400, seed=0, th=3.0, ratio=1.5, n_claimed=20, **fuse_args):
    """One keyframe and n_mp MapPoints for ORBmatcher.SearchByProjectionSim3: the one-keyframe
    synthetic_fuse_scene of the first ceil(3 n_mp / 4) points, and behind them a copy of every third
    of those points (position, normal, range and descriptor), so that a copy competes with its
    original for the same keypoints and, coming later in the list, loses its first choice.
    n_claimed keypoints (fewer when the keyframe has fewer) are claimed at call time (vpMatched set).
    The keyframe's pose stands for Tcw = (R, t / s) of the Sim3 the adapter decomposed. Returns a
    dict: kf (ProjFrame with claimed), points, normals, min_dist, max_dist, mp_desc, skip, th, ratio,
    kind, copy_of (-1 for an original)."""
    from .matcher import ProjFrame
    base = (3 * n_mp + 3) // 4
    s = synthetic_fuse_scene(n_kp, base, 1, seed, th=th, **fuse_args)
    src = 3 * np.arange(n_mp - base)
    assert src.size == 0 or src[-1] < base
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    k0 = s["kfs"][0]
    nk = k0.kps.shape[0]
    claimed = np.zeros(nk, np.uint8)
    claimed[rng.choice(nk, min(n_claimed, nk), replace=False)] = 1
    kf = ProjFrame(k0.kps, k0.desc, k0.pose_q, k0.pose_t, k0.fx, k0.fy, k0.cx, k0.cy, *k0.bounds[1::2],
                   claimed=claimed)
    kf.scale_factors, kf.log_scale_factor = k0.scale_factors, k0.log_scale_factor
    out = {k: np.concatenate([s[k], s[k][src]]) for k in ("points", "normals", "min_dist", "max_dist", "mp_desc",
                                                          "skip", "kind")}
    out.update(kf=kf, th=float(th), ratio=float(ratio), scale_factors=s["scale_factors"],
               inv_level_sigma2=s["inv_level_sigma2"], copy_of=np.concatenate([np.full(base, -1), src]))
    return out


# ---------------------------------------------------------------------------
# Rectified-stereo tracking: PoseOptimization with stereo edges, the stereo branches of the
# projection matchers
# ---------------------------------------------------------------------------
STEREO_B = 0.08                                                    # mb, metres


def synthetic_stereo_pose_problem(n=600, outlier_frac=0.15, seed=3, stereo_frac=0.5, ur_outlier_frac=0.06,
                                  b=STEREO_B, **pose_args):
    """synthetic_pose_problem(n, outlier_frac, seed, ...) seen by a rectified-stereo Frame: about
    stereo_frac of the observations carry u_right = the projection into the right image (u - bf / z,
    bf = fx * b) + 1.2^octave px noise, the others -1 (monocular). A gross mismatch keeps a right
    coordinate consistent with its own (wrong) keypoint at a random depth; ur_outlier_frac of the
    good stereo observations get a right coordinate 4-15 sigma off (a wrong stereo match: an outlier
    as a stereo edge only). A right coordinate that would be negative is dropped (-1).
    Returns (PoseProblem with u_right / bf, ground truth dict + stereo, ur_bad masks)."""
    prob, gt = synthetic_pose_problem(n=n, outlier_frac=outlier_frac, seed=seed, **pose_args)
    rng = np.random.Generator(np.random.PCG64(7919 * (seed + 1) + 17))
    fx = float(np.float32(prob.fx))
    bf = float(np.float32(fx * b))
    Xc = prob.points.astype(np.float64) @ gt["R"].T + gt["t"]
    z = Xc[:, 2]
    sig = np.power(1.2, prob.octave.astype(np.float64))
    u_true = fx * Xc[:, 0] / z + float(np.float32(prob.cx))
    ur = u_true - bf / z + rng.normal(size=n) * sig
    bad = gt["bad"]
    ur[bad] = prob.uv[bad, 0].astype(np.float64) - bf / rng.uniform(2.0, 6.0, int(bad.sum()))
    stereo = rng.random(n) < stereo_frac
    ur_bad = stereo & ~bad & (rng.random(n) < ur_outlier_frac)
    ur[ur_bad] += rng.choice([-1.0, 1.0], int(ur_bad.sum())) * rng.uniform(4.0, 15.0, int(ur_bad.sum())) * sig[ur_bad]
    stereo &= ur >= 0.5
    ur_bad &= stereo
    prob.u_right = np.where(stereo, ur, -1.0).astype(np.float32)
    prob.bf = bf
    return prob, dict(gt, stereo=stereo, ur_bad=ur_bad)


def synthetic_stereo_projection_scene(n_kp=1000, n_mp=900, seed=5, motion="forward", b=STEREO_B, mono_frac=0.2,
                                      wrong_frac=0.25, level_frac=0.8, **scene_args):
    """synthetic_projection_scene(n_kp, n_mp, seed, ...) seen by a rectified-stereo Frame, plus the
    last frame's pose. Every keypoint gets u_right = x - bf / z (bf = fx * b) + a quarter pixel of
    noise, z the depth of the first MapPoint made from it (1-8 m at random for the others; the other
    MapPoints stacked on one keypoint have depths of their own, so the gate tells them apart);
    mono_frac have no stereo match (-1), wrong_frac a wrong one (30-120 px off: the gate rejects the
    true candidate and the query falls to its next best). level_frac of the MapPoints get distance
    bounds that predict their keypoint's octave or the one above (the base scene's are random, so few
    of its points pass SearchLocalPoints' level window and the gate would have little to reject). The
    last frame looks the same way from 0.3 m behind (motion 'forward': tlc.z > b), 0.3 m ahead
    ('backward') or 2 cm aside ('neutral').
    Returns the base scene's dict + u_right, bf, b, last_pose_q, last_pose_t, direction."""
    s = synthetic_projection_scene(n_kp=n_kp, n_mp=n_mp, seed=seed, **scene_args)
    rng = np.random.Generator(np.random.PCG64(104729 * (seed + 1) + 5))
    if n_mp:
        Ow = -quat_to_rot64(s["pose_q"]).T @ s["pose_t"].astype(np.float64)
        dist = np.linalg.norm(s["points"].astype(np.float64) - Ow, axis=1)
        lvl = s["kps"]["octave"][s["src"]] + rng.integers(0, 2, n_mp) - rng.uniform(0.1, 0.9, n_mp)
        fit = rng.random(n_mp) < level_frac
        n_levels = scene_args.get("n_levels", 8)
        max_dist = dist * np.power(1.2, lvl)
        s["max_dist"] = np.where(fit, max_dist.astype(np.float32), s["max_dist"])
        s["min_dist"] = np.where(fit, (max_dist / np.float64(1.2) ** (n_levels - 1)).astype(np.float32), s["min_dist"])
    fx = float(np.float32(s["fx"]))
    bf = float(np.float32(fx * b))
    q, t = s["pose_q"], s["pose_t"]
    R = quat_to_rot64(q)
    zk = rng.uniform(1.0, 8.0, n_kp)
    if n_mp:
        zmp = (s["points"].astype(np.float64) @ R.T + t.astype(np.float64))[:, 2]
        first = np.full(n_kp, -1)
        for m in range(n_mp - 1, -1, -1):
            first[s["src"][m]] = m
        has = first >= 0
        zk[has] = zmp[first[has]]
    ur = s["kps"]["x"].astype(np.float64) - bf / zk + rng.normal(size=n_kp) * 0.25
    wrong = rng.random(n_kp) < wrong_frac
    ur[wrong] += rng.choice([-1.0, 1.0], int(wrong.sum())) * rng.uniform(30.0, 120.0, int(wrong.sum()))
    none = (rng.random(n_kp) < mono_frac) | (ur < 0.5)
    u_right = np.where(none, -1.0, ur).astype(np.float32)
    tlc = dict(forward=np.array([0.01, -0.02, 0.3]), backward=np.array([-0.02, 0.01, -0.3]),
               neutral=np.array([0.02, 0.005, 0.02]))[motion]
    Rl = _rodrigues(rng.normal(size=3) * 0.01) @ R
    ql = _mat_to_quat(Rl).astype(np.float32)
    twc = -R.T @ t.astype(np.float64)
    tl = (tlc - quat_to_rot64(ql) @ twc).astype(np.float32)
    return dict(s, u_right=u_right, bf=bf, b=float(np.float32(b)), last_pose_q=ql, last_pose_t=tl,
                direction=dict(forward=1, backward=-1, neutral=0)[motion])


def synthetic_stereo_new_points_scene(n=300, B=3, seed=0, b=STEREO_B, scale=0.3, mono_frac=0.3, off_frac=0.06,
                                      zero_depth_frac=0.015, gated_at=1, **scene_args):
    """synthetic_new_points_scene(n, B, seed, scale=scale, ...) seen by rectified-stereo keyframes, for
    the stereo branches of SearchForTriangulation / CreateNewMapPoints. scale = 0.3 puts the
    neighbours 0.09-0.14 m from KF1 and the points 0.6-2.4 m away, so that against a stereo baseline
    b = 0.08 m the ray parallax wins for the sideways neighbour (triangulated), loses for most of the
    forward one (unprojected) and the diagonal one has both. A KF1 feature's depth is that of the
    float64 triangulation with its twin in the first (sideways) neighbour (1-8 scaled metres at
    random without one), a twin's depth that of the same point in its own camera; u_right = x - bf /
    depth (bf = fx * b) + 0.15 level sigma of noise. Then, per feature of every keyframe:
      mono_frac        lose the stereo members (u_right = depth = -1; also where u_right < 0.5)
      off_frac         of the stereo features get a right coordinate 4-8 level sigma off (depth kept):
                       the three-term reprojection test fails where the monocular one passes
      zero_depth_frac  of the stereo features get depth 0 (UnprojectStereo refuses them)
    The neighbour inserted at gated_at lies 1 mm * scale from KF1: below every b, gated. Draws come
    from a generator of their own. Returns the base dict with kf1 / neighbours carrying u_right, depth,
    bf, b, plus b, bf, mono_kf1 / mono_neighbours (the same keyframes without them); median_depth is
    None (the stereo call has no such gate)."""
    from .matcher import TriKeyFrame
    cam = dict(scene_args.pop("cam", None) or WIDE_CAM)
    s = synthetic_new_points_scene(n, B, seed, cam=cam, scale=scale, gated_at=gated_at, **scene_args)
    twins = synthetic_triangulation_scene(n, B, seed, cam=cam, **scene_args)["twin"]
    rng = np.random.Generator(np.random.PCG64(32452843 * (seed + 1) + 7))
    m = float(scale)
    sf = s["scale_factors"].astype(np.float64)
    k1, nbrs = s["kf1"], s["neighbours"]
    bf = float(np.float32(np.float32(cam["fx"]) * np.float32(b)))
    R1, t1 = _pose64(k1)

    def tri_depth(k2, p1, p2):   # depth in KF1 of the float64 triangulation of two pixels
        rows = []
        for k, p in ((k1, p1), (k2, p2)):
            R, t = _pose64(k)
            T = np.concatenate([R, t[:, None]], 1)
            xn = ((p[0] - k.cx) / k.fx, (p[1] - k.cy) / k.fy)
            rows += [xn[0] * T[2] - T[0], xn[1] * T[2] - T[1]]
        v = np.linalg.svd(np.array(rows))[2][3]
        if v[3] == 0:
            return -1.0
        return float((R1 @ (v[:3] / v[3]) + t1)[2])

    def new_index(bb):           # a base neighbour's place in the list with the gated one
        return bb + (gated_at is not None and B > 0 and bb >= gated_at)

    z1 = rng.uniform(1.0, 8.0, k1.n) * m
    if B > 0:
        k2 = nbrs[new_index(0)]
        for i in np.nonzero(twins[0] >= 0)[0]:
            j = int(twins[0][i])
            z = tri_depth(k2, (k1.kps["x"][i], k1.kps["y"][i]), (k2.kps["x"][j], k2.kps["y"][j]))
            if 0.3 * m < z < 30.0 * m:
                z1[i] = z
    Xw = (np.stack([(k1.kps["x"] - cam["cx"]) / cam["fx"] * z1, (k1.kps["y"] - cam["cy"]) / cam["fy"] * z1, z1], 1)
          - t1) @ R1
    depths = [z1]
    for a, k in enumerate(nbrs):
        z = rng.uniform(1.0, 8.0, k.n) * m
        base_b = [bb for bb in range(B) if new_index(bb) == a]
        if base_b:
            R, t = _pose64(k)
            zc = (Xw @ R.T + t)[:, 2]
            tw = twins[base_b[0]]
            for i in np.nonzero(tw >= 0)[0]:
                if tw[i] < k.n and zc[i] > 0.1 * m:
                    z[int(tw[i])] = zc[i]
        depths.append(z)

    def dress(k, z):
        nk = k.n
        sig = sf[k.kps["octave"]]
        ur = k.kps["x"].astype(np.float64) - bf / z + rng.normal(size=nk) * 0.15 * sig
        mono = rng.random(nk) < mono_frac
        kind = rng.random(nk)
        off = kind < off_frac
        ur[off] += rng.choice([-1.0, 1.0], int(off.sum())) * rng.uniform(4.0, 8.0, int(off.sum())) * sig[off]
        mono |= ur < 0.5
        z = np.where((kind >= off_frac) & (kind < off_frac + zero_depth_frac), 0.0, z)
        u_right = np.where(mono, -1.0, ur).astype(np.float32)
        depth = np.where(mono, -1.0, z).astype(np.float32)
        return TriKeyFrame(k.kps, k.desc, k.node, k.weight, k.has_mp, k.pose_q, k.pose_t, k.fx, k.fy, k.cx, k.cy,
                           u_right=u_right, depth=depth, bf=bf, b=float(np.float32(b)))

    stereo = [dress(k, z) for k, z in zip([k1] + nbrs, depths)]
    return dict(s, kf1=stereo[0], neighbours=stereo[1:], mono_kf1=k1, mono_neighbours=nbrs, median_depth=None,
                b=float(np.float32(b)), bf=bf)


def synthetic_stereo_fuse_scene(n_kp=300, n_mp=300, B=3, seed=0, b=STEREO_B, mono_frac=0.25, off_frac=0.12,
                                ring_frac=0.1, **fuse_args):
    """synthetic_fuse_scene(n_kp, n_mp, B, seed, ...) seen by rectified-stereo keyframes, for the
    stereo branch of ORBmatcher.Fuse. A keypoint is tied to the MapPoint whose projection into its
    keyframe lies nearest, when that is within 4 level sigma (sigma = mvScaleFactors[octave]); tied
    keypoints get u_right = that point's right projection u - bf / z (bf = fx * b) + 0.15 sigma of
    noise, the others one for a depth of 1-8 m. Then, independently per keypoint:
      mono_frac   lose the right coordinate (-1: a monocular keypoint; also where it would be < 0)
      off_frac    of the tied stereo keypoints get a right coordinate 3-6 sigma off: with a small
                  (u, v) error the three-term chi-square rejects what the monocular test accepts
      ring_frac   of the tied stereo keypoints are moved onto a ring 2.5-2.7 sigma from the
                  projection, the right coordinate kept: rejected at 5.99, accepted at 7.8
    The draws come from a generator of their own and the points are the base scene's, so its level
    margin holds. Returns the base scene's dict with kfs replaced by ProjFrames that carry u_right /
    bf / b, plus bf, b and mono_kfs (the same keyframes, moved keypoints included, without them)."""
    from .matcher import ProjFrame
    s = synthetic_fuse_scene(n_kp, n_mp, B, seed, **fuse_args)
    rng = np.random.Generator(np.random.PCG64(15485863 * (seed + 1) + 11))
    sf = s["scale_factors"].astype(np.float64)
    P64 = s["points"].astype(np.float64)
    kfs, mono_kfs = [], []
    bf = 0.0
    for k in s["kfs"]:
        cam = dict(fx=k.fx, fy=k.fy, cx=k.cx, cy=k.cy)
        bf = float(np.float32(np.float32(k.fx) * np.float32(b)))
        nk = k.kps.shape[0]
        kps = k.kps.copy()
        x, y = kps["x"].astype(np.float64), kps["y"].astype(np.float64)
        sig = sf[kps["octave"]]
        tied = np.zeros(nk, bool)
        pu, pv, pz = np.zeros(nk), np.zeros(nk), rng.uniform(1.0, 8.0, nk)
        if n_mp:
            with np.errstate(all="ignore"):
                uv, z = pinhole_project(k.pose_q, k.pose_t, cam, P64)
            front = z > 0.1
            for i0 in range(0, nk, 256):
                i1 = min(nk, i0 + 256)
                d2 = (x[i0:i1, None] - uv[None, :, 0]) ** 2 + (y[i0:i1, None] - uv[None, :, 1]) ** 2
                d2[:, ~front] = np.inf
                m = np.argmin(d2, axis=1)
                near = np.sqrt(d2[np.arange(i1 - i0), m]) < 4.0 * sig[i0:i1]
                tied[i0:i1] = near
                pu[i0:i1], pv[i0:i1] = uv[m, 0], uv[m, 1]
                pz[i0:i1] = np.where(near, z[m], pz[i0:i1])
        ur = np.where(tied, pu, x) - bf / pz + rng.normal(size=nk) * 0.15 * sig
        mono = (rng.random(nk) < mono_frac) | (ur < 0.5)
        kind = rng.random(nk)
        off = tied & ~mono & (kind < off_frac)
        ring = tied & ~mono & (kind >= off_frac) & (kind < off_frac + ring_frac)
        ur[off] += rng.choice([-1.0, 1.0], int(off.sum())) * rng.uniform(3.0, 6.0, int(off.sum())) * sig[off]
        mono |= ur < 0.5
        a, rho = rng.uniform(0, 2 * np.pi, nk), rng.uniform(2.5, 2.7, nk) * sig
        kps["x"] = np.where(ring, pu + rho * np.cos(a), x).astype(np.float32)
        kps["y"] = np.where(ring, pv + rho * np.sin(a), y).astype(np.float32)
        u_right = np.where(mono, -1.0, ur).astype(np.float32)
        for out, extra in ((kfs, dict(u_right=u_right, bf=bf, b=float(np.float32(b)))), (mono_kfs, {})):
            f = ProjFrame(kps, k.desc, k.pose_q, k.pose_t, k.fx, k.fy, k.cx, k.cy, bounds=k.bounds, **extra)
            f.scale_factors, f.log_scale_factor = k.scale_factors, k.log_scale_factor
            out.append(f)
    return dict(s, kfs=kfs, mono_kfs=mono_kfs, bf=bf, b=float(np.float32(b)))


def synthetic_stereo_ba_problem(n_kf=50, n_pts=2000, stereo_frac=0.7, seed=7, ur_noise=1.0, b=0.05, **ba_args):
    """synthetic_ba_problem(n_kf, n_pts, seed=seed, ...) seen by rectified-stereo keyframes: about
    stereo_frac of the observations carry edge_ur = the ground-truth point's projection into the
    right image (u - bf / z, bf = fx * b, a 50 mm baseline) + ur_noise * 1.2^octave px of noise, the
    others -1 (monocular edges). A right coordinate that would be negative is dropped (-1). The
    stereo draws come from a generator of their own, so the monocular problem's arrays are those of
    synthetic_ba_problem for the same seed.
    Returns (StereoBAProblem with perturbed initial state, ground-truth dict + `stereo`, the mask of
    the stereo edges, and `ur`, every edge's right coordinate before the mask)."""
    from .optimizer import StereoBAProblem, TH_HUBER_STEREO
    prob, gt = synthetic_ba_problem(n_kf=n_kf, n_pts=n_pts, seed=seed, **ba_args)
    rng = np.random.Generator(np.random.PCG64(104729 * (seed + 1) + 31))
    E = prob.edge_pose.shape[0]
    fx = float(np.float32(prob.fx))
    bf = float(np.float32(fx * b))
    Xc = np.einsum("eij,ej->ei", gt["R"][prob.edge_pose], gt["points"][prob.edge_point]) + gt["t"][prob.edge_pose]
    z = Xc[:, 2]
    sig = np.power(np.float64(ba_args.get("scale_factor", 1.2)), prob.edge_octave.astype(np.float64))
    stereo = rng.random(E) < stereo_frac
    ur = fx * Xc[:, 0] / z + float(np.float32(prob.cx)) - bf / z + rng.normal(size=E) * sig * ur_noise
    stereo &= ur >= 0.0
    sp = StereoBAProblem(**prob.__dict__, edge_ur=np.where(stereo, ur, -1.0).astype(np.float32), bf=bf,
                         huber_delta_stereo=TH_HUBER_STEREO)
    return sp, dict(gt, stereo=stereo, ur=ur)


# ---------------------------------------------------------------------------
# Sim3Solver scenes (LoopClosing::DetectCommonRegionsFromBoW)
# ---------------------------------------------------------------------------
def synthetic_sim3_solver_scene(n=100, outlier_frac=0.5, seed=0, fix_scale=False, n_hyp=300, min_inliers=15,
                                n_levels=8, scale_factor=1.2, noise_px=0.7, cam1=None, cam2=None, n_degenerate=2):
    """What Sim3Solver's constructor leaves of a loop candidate: n correspondences X1 / X2 (the map
    points in the two cameras' frames, float32) with points in front of camera 1, a true Sim3
    (X1 = s R X2 + t; s = 1 when the scale is fixed), noise of noise_px pixels at each point's depth,
    a share of the X2 replaced by unrelated points (outliers), random octaves and with them upstream's
    truncated error bounds, and n_hyp triples drawn by draw_triples from a seeded generator. Also
    indices1 / n1 (mvnIndices1, mN1), the true (s, R, t), and n_degenerate planted hypotheses
    (degenerate_h) whose three correspondences are copies of one."""
    from .sim3solver import draw_triples, error_bounds
    rng = np.random.default_rng(seed)
    c1 = dict(D435I) if cam1 is None else dict(cam1)
    c2 = dict(fx=600.0, fy=605.0, cx=318.5, cy=242.25) if cam2 is None else dict(cam2)
    X1 = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 8.0, n)], 1)
    R = _rodrigues(rng.normal(size=3) * 0.12)
    t = rng.normal(size=3) * 0.25
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    X2 = (X1 - t) @ R / s                      # rows: R^T (X1 - t) / s
    out = rng.random(n) < outlier_frac
    X2[out] = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.0, 9.0, n)], 1)[out]
    for X, c in ((X1, c1), (X2, c2)):          # pixel noise at the point's depth, and a little in depth
        X[:, 0] += rng.normal(size=n) * noise_px * X[:, 2] / c["fx"]
        X[:, 1] += rng.normal(size=n) * noise_px * X[:, 2] / c["fy"]
        X[:, 2] *= 1.0 + rng.normal(size=n) * 1e-3
    _, s2 = orb_scale_tables(n_levels, scale_factor)
    oct1, oct2 = rng.integers(0, n_levels, n), rng.integers(0, n_levels, n)
    n1 = n + n // 3
    indices1 = np.sort(rng.choice(n1, n, replace=False))
    draw = np.random.default_rng(seed + 7919)
    triples = draw_triples(n, n_hyp, lambda lo, hi: int(draw.integers(lo, hi + 1)))
    # degenerate hypotheses: three correspondences that coincide (M = 0: NaN scale when it is free),
    # their triple planted at two places
    degenerate_h = []
    if n_degenerate and n >= 6 and n_hyp >= 4:
        pool = np.nonzero(out)[0] if out.sum() >= 3 else np.arange(n)   # outliers: the counts hardly move
        i0, i1, i2 = (int(i) for i in rng.choice(pool, 3, replace=False))
        X1[[i1, i2]], X2[[i1, i2]] = X1[i0], X2[i0]
        degenerate_h = [1, n_hyp // 2][:n_degenerate]
        triples[degenerate_h] = (i0, i1, i2)
    cams =[np.array([c[k] for k in ("fx", "fy", "cx", "cy")], np.float32) for c in (c1, c2)]
    return dict(X1=X1.astype(np.float32), X2=X2.astype(np.float32), octaves1=oct1, octaves2=oct2,
                level_sigma2=s2, max_err1=error_bounds(oct1, s2), max_err2=error_bounds(oct2, s2),
                cam1=cams[0], cam2=cams[1], fix_scale=bool(fix_scale), min_inliers=int(min_inliers),
                triples=triples, indices1=indices1, n1=n1, outlier=out, degenerate_h=degenerate_h, true_s=s, true_R=R, true_t=t)


# ---------------------------------------------------------------------------
# OptimizeSim3 problems (LoopClosing's Sim3 refinement)
# ---------------------------------------------------------------------------
def synthetic_sim3_opt_problem(n=100, outlier_frac=0.2, seed=0, fix_scale=False, proj_frac=0.0, noise_px=0.7,
                               rot_noise=0.02, trans_noise=0.05, scale_noise=0.03, n_levels=8, scale_factor=1.2,
                               cam1=None, cam2=None):
    """What OptimizeSim3's filter loop leaves of two keyframes that see the same n map points: X1c /
    X2c (the points in the two cameras' frames, float32) under a true Sim3 X1 = s R X2 + t (s = 1 when
    the scale is fixed), keypoints = the projections plus noise_px pixels scaled by each keypoint's
    octave, and with the octaves the information values. A share outlier_frac of the pairs are gross
    mismatches (the keypoint in KF1 moved by 25 to 80 pixels); a share proj_frac of the others have no
    keypoint in KF2 (upstream's i2 < 0 with bAllPoints) and get upstream's obs2 for them: the NORMALISED
    x / z, y / z of the point and the information of a track level. The initial S12 is the true one
    moved by rot_noise rad, trans_noise and a relative scale_noise (no scale change when fixed).
    Returns (Sim3Problem, dict(R, t, s, bad = mismatch or without keypoint, by_projection))."""
    from .optimizer import Sim3Problem
    rng = np.random.default_rng(seed)
    c1 = dict(D435I) if cam1 is None else dict(cam1)
    c2 = dict(fx=600.0, fy=605.0, cx=318.5, cy=242.25) if cam2 is None else dict(cam2)
    X1 = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 8.0, n)], 1)
    R = _rodrigues(rng.normal(size=3) * 0.12)
    t = rng.normal(size=3) * 0.25
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    X2 = (X1 - t) @ R / s                      # rows: R^T (X1 - t) / s
    X1f, X2f = X1.astype(np.float32), X2.astype(np.float32)
    _, s2 = orb_scale_tables(n_levels, scale_factor)
    oct1, oct2 = rng.integers(0, n_levels, n), rng.integers(0, n_levels, n)
    obs = []
    for X, c, o in ((X1f.astype(np.float64), c1, oct1), (X2f.astype(np.float64), c2, oct2)):
        sd = noise_px * np.sqrt(s2[o])
        obs.append(np.stack([c["fx"] * X[:, 0] / X[:, 2] + c["cx"] + rng.normal(size=n) * sd,
                             c["fy"] * X[:, 1] / X[:, 2] + c["cy"] + rng.normal(size=n) * sd], 1))
    bad = rng.random(n) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, n)
    obs[0][bad] += (rng.uniform(25.0, 80.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[bad]
    by_proj = (rng.random(n) < proj_frac) & ~bad
    z2 = X2f[:, 2:3].astype(np.float64)
    obs[1][by_proj] = (X2f[:, :2].astype(np.float64) / z2)[by_proj]
    R0 = _rodrigues(rng.normal(size=3) * rot_noise) @ R
    t0 = t + rng.normal(size=3) * trans_noise
    s0 = s if fix_scale else s * (1.0 + float(rng.normal()) * scale_noise)
    cams = [np.array([c[k] for k in ("fx", "fy", "cx", "cy")], np.float32) for c in (c1, c2)]
    prob = Sim3Problem(X1f, X2f, obs[0].astype(np.float32), obs[1].astype(np.float32),
                       (1.0 / s2[oct1]).astype(np.float32), (1.0 / s2[oct2]).astype(np.float32), cams[0], cams[1],
                       _mat_to_quat(R0), t0, float(s0), 10.0, bool(fix_scale))
    return prob, dict(R=R, t=t, s=s, bad=bad | by_proj, by_projection=by_proj)


# ---------------------------------------------------------------------------
# OptimizeEssentialGraph problems (CorrectLoop's pose graph)
# ---------------------------------------------------------------------------
def _s3(R, t, s):
    """(R, t, s) as a g2o::Sim3 row: Eigen's quaternion (x, y, z, w), t, s."""
    return np.concatenate([_mat_to_quat(R), np.asarray(t, np.float64), [float(s)]])


def _s3_parts(a):
    x, y, z, w = a[0:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, a[4:7], a[7]


def _s3_mul(a, b):
    Ra, ta, sa = _s3_parts(a)
    Rb, tb, sb = _s3_parts(b)
    return _s3(Ra @ Rb, sa * (Ra @ tb) + ta, sa * sb)


def _s3_inv(a):
    R, t, s = _s3_parts(a)
    return _s3(R.T, -(R.T @ t) / s, 1.0 / s)


def synthetic_essential_graph(n_kf=100, k_covis=3, loop_span=5, drift=0.01, scale_drift=0.002, fix_scale=False,
                              seed=0, n_points=0):
    """The graph CorrectLoop hands to OptimizeEssentialGraph after a loop over n_kf keyframes on a
    closed trajectory (a circle of radius 5 looking along the motion). The tracked poses accumulate a
    Sim3 drift per step: `drift` rad of rotation, `drift` of the step length in translation and a
    relative `scale_drift` of the map's scale (none when fix_scale). Vertices are in keyframe-id order
    and keyframe 0 is fixed. The last loop_span keyframes (the current keyframe's neighbourhood) carry
    corrected estimates (upstream's CorrectedSim3: Sic * Scw_corrected, the loop's Sim3 carried
    through the tracked relative poses), every other one its tracked SE3 pose as a Sim3 with s = 1.
    Edges, each (i, j, Sji) with i > j: the chain spanning tree (i, i - 1), covisibility edges to the
    k_covis keyframes before the parent, both measured from the tracked (non-corrected) poses as
    upstream computes Sji = Sjw * Swi; and loop-connection edges from the last loop_span keyframes to
    the first ones, measured from the estimates (upstream's vScw). n_points map points hang off random
    reference keyframes, in front of their tracked cameras. Returns (EssentialGraphProblem,
    dict(true = the true Scw rows, tracked = the non-corrected rows, corrected = the corrected ids))."""
    from .optimizer import EssentialGraphProblem
    rng = np.random.default_rng(seed)
    n = int(n_kf)
    span = max(1, min(int(loop_span), n // 2))
    ang = 2 * np.pi * np.arange(n) / n
    true = []
    for a in ang:   # camera at (5 cos a, 0, 5 sin a), z along the tangent
        zc = np.array([-np.sin(a), 0.0, np.cos(a)])
        yc = np.array([0.0, 1.0, 0.0])
        xc = np.cross(yc, zc)
        Rwc = np.stack([xc, yc, zc], 1)
        twc = np.array([5 * np.cos(a), 0.0, 5 * np.sin(a)])
        true.append(_s3(Rwc.T, -Rwc.T @ twc, 1.0))
    tracked = [true[0].copy()]
    sc = 1.0
    for k in range(1, n):
        rel = _s3_mul(true[k], _s3_inv(true[k - 1]))
        R, t, _ = _s3_parts(rel)
        if not fix_scale:
            sc *= 1.0 + scale_drift * float(rng.normal())
        Rn = _rodrigues(rng.normal(size=3) * drift) @ R
        tn = sc * t + rng.normal(size=3) * drift * np.linalg.norm(t)
        tracked.append(_s3_mul(_s3(Rn, tn, 1.0), tracked[k - 1]))
    cur = n - 1
    Rc, tc, _ = _s3_parts(true[cur])
    Scw = _s3(Rc, sc * tc, sc)            # the loop's Sim3 of the current keyframe
    S = [t.copy() for t in tracked]
    corrected = list(range(n - span, n))
    for i in corrected:
        S[i] = _s3_mul(_s3_mul(tracked[i], _s3_inv(tracked[cur])), Scw)
    ij, Sji = [], []
    for i in range(1, n):
        for j in range(i - 1, max(-1, i - 2 - int(k_covis)), -1):
            ij.append((i, j))
            Sji.append(_s3_mul(tracked[j], _s3_inv(tracked[i])))
    for a, i in enumerate(corrected):
        for j in (a, a + 1):
            if j < span and j < n - span:
                ij.append((i, j))
                Sji.append(_s3_mul(S[j], _s3_inv(S[i])))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    pts, ref = None, None
    if n_points:
        ref = rng.integers(0, n, int(n_points)).astype(np.int32)
        Xc = np.stack([rng.uniform(-1.5, 1.5, n_points), rng.uniform(-1.0, 1.0, n_points),
                       rng.uniform(2.0, 6.0, n_points)], 1)
        pts = np.empty((int(n_points), 3), np.float32)
        for m in range(int(n_points)):
            R, t, s = _s3_parts(_s3_inv(tracked[ref[m]]))
            pts[m] = s * (R @ Xc[m]) + t
    prob = EssentialGraphProblem(np.array(S), fixed, np.array(ij, np.int32).reshape(-1, 2),
                                 np.array(Sji).reshape(-1, 8), bool(fix_scale), 20, 1e-16, pts, ref)
    return prob, dict(true=np.array(true), tracked=np.array(tracked), corrected=corrected)


# ---------------------------------------------------------------------------
# TwoViewReconstruction problems (monocular initialisation)
# ---------------------------------------------------------------------------
def synthetic_two_view_scene(kind="general", n=300, seed=0, outlier_frac=0.1, noise_px=0.3, unmatched_frac=0.0,
                             n_hyp=200, sigma=1.0, cam=None, doubled=False, plane=(5.0, 0.25, -0.15),
                             t_mean=(0.45, 0.05, 0.08)):
    """What Tracking::MonocularInitialization hands to TwoViewReconstruction::Reconstruct: the
    undistorted keypoints of two frames (x, y; float32), vMatches12 (n1 entries, -1 = unmatched), K
    as (fx, fy, cx, cy), and n_hyp 8-sets drawn by draw_sets from a seeded generator. n matches; kind:
    "general" (points in a volume, a sideways baseline), "planar" (points on a tilted plane),
    "mixed" (half on the plane, half in the volume), "rotation" (no baseline) or "low_parallax" (a
    baseline of a thousandth of the depth). A share outlier_frac of the matches point at unrelated
    places of frame 2, the inliers carry noise_px pixels of noise, and a share unmatched_frac of extra
    keypoints of frame 1 have no match. Also the true (R21, t21 with unit norm) and the outlier flags
    per match.

    doubled: every match occurs twice (matches 2k and 2k + 1 have equal coordinates, as keypoints
    found on two pyramid levels do) and every set holds four such twins. Four distinct points fix a
    homography but leave the fundamental matrix's system five null directions, so its hypotheses are
    poor: with upstream's RH > 0.50 this is how a homography wins, which it never does when both
    models are fitted to sound sets (CheckFundamental rejects less than CheckHomography)."""
    from .two_view import draw_sets
    rng = np.random.default_rng(seed)
    c = dict(D435I) if cam is None else dict(cam)
    fx, fy, cx, cy = (float(c[k]) for k in ("fx", "fy", "cx", "cy"))
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 9.0, n)], 1)
    plane = plane[0] + plane[1] * X[:, 0] + plane[2] * X[:, 1]   # z = z0 + a x + b y
    if kind == "planar":
        X[:, 2] = plane
    elif kind == "mixed":
        X[::2, 2] = plane[::2]
    R = _rodrigues(np.array([0.02, -0.05, 0.03]) + rng.normal(size=3) * 0.01)
    t = np.array(t_mean, float) + rng.normal(size=3) * 0.02
    if kind == "rotation":
        t = np.zeros(3)
    elif kind == "low_parallax":
        t = t * 0.01
    elif kind not in ("general", "planar", "mixed"):
        raise ValueError(f"unknown kind {kind!r}")
    X2 = X @ R.T + t
    p1 = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    p1 += rng.normal(size=p1.shape) * noise_px
    p2 += rng.normal(size=p2.shape) * noise_px
    out = rng.random(n) < outlier_frac
    p2[out] = np.stack([rng.uniform(20.0, 2 * cx - 20.0, n), rng.uniform(20.0, 2 * cy - 20.0, n)], 1)[out]
    if doubled:
        if n % 2 or n < 8:
            raise ValueError("doubled needs an even n >= 8")
        p1[1::2], p2[1::2], out[1::2] = p1[0::2], p2[0::2], out[0::2]
    n_extra = int(round(unmatched_frac * n))
    n1 = n + n_extra
    slots = np.sort(rng.choice(n1, n, replace=False))          # the matched keypoints of frame 1
    kps1 = np.stack([rng.uniform(20.0, 2 * cx - 20.0, n1), rng.uniform(20.0, 2 * cy - 20.0, n1)], 1)
    kps1[slots] = p1
    perm = rng.permutation(n)                                   # frame 2 holds them in another order
    kps2 = np.empty((n, 2))
    kps2[perm] = p2
    matches12 = np.full(n1, -1, np.int32)
    matches12[slots] = perm
    draw = np.random.default_rng(seed + 7919)
    sets = draw_sets(n, n_hyp, lambda lo, hi: int(draw.integers(lo, hi + 1)))
    if doubled:
        twins = draw_sets(n // 2, n_hyp, lambda lo, hi: int(draw.integers(lo, hi + 1)))[:, :4]
        sets = np.stack([2 * twins, 2 * twins + 1], 2).reshape(n_hyp, 8).astype(np.int32)
    nt = np.linalg.norm(t)
    return dict(kps1=kps1.astype(np.float32), kps2=kps2.astype(np.float32), matches12=matches12,
                K=np.array([fx, fy, cx, cy], np.float32), sigma=float(sigma), sets=sets, outlier=out,
                true_R=R, true_t=t / nt if nt > 0 else t, kind=kind)
