"""The numpy mirror of csrc/map_covis.hip (the rule: include/gsloc_hip.h, "covisibility"): the verdicts of
tests/map_score_ref.py for one pose, binned by the origin of every row with ``np.add.at`` -- the origin is looked at
first: a row whose origin lies outside the table is counted as outside and nowhere else, whatever its mean is."""
import numpy as np

from tests.map_score_ref import verdicts

F32 = np.float32


def covis(means, origins, w2c, intr, depth, keep, beyond, near, n_frames):
    """means [n,3] float32, origins [n] int32 -> (counts int64 [n_frames,3] = per frame (rows tested, rows that agree,
    rows in front), rows whose origin is < 0 or >= n_frames)."""
    o = np.asarray(origins, np.int64).reshape(-1)
    p = np.asarray(means, F32).reshape(-1, 3)
    assert len(o) == len(p) and n_frames >= 1
    outside = (o < 0) | (o >= n_frames)
    tested, agree, front, _ = verdicts(p, w2c, intr, depth, keep, beyond, near)
    counts = np.zeros((n_frames, 3), np.int64)
    for j, verdict in enumerate((tested, agree, front)):
        np.add.at(counts[:, j], o[~outside & verdict], 1)
    return counts, int(outside.sum())


def room_loop_map(width=160, height=120):
    """The room loop of tests/map_correct_ref.room_loop(): (rows [8 W H, 3] float32, origins int32, true poses, drifted
    poses, depth images [8][H,W] float32, intrinsics (fx, fy, cx, cy), K) -- every frame inserted whole, its pixels
    back-projected in float64 at its DRIFTED pose and rounded to float32 once, in raster order."""
    import torch

    from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
    from tests import map_correct_ref

    K = replica_intrinsics(width, height)
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    true, est = map_correct_ref.room_loop()
    depths = [room_depth(width, height, K, torch.from_numpy(p).float()).numpy() for p in true]
    v, u = np.mgrid[0:height, 0:width]
    rows, origins = [], []
    for k, d in enumerate(depths):
        cam = np.stack([(u - intr[2]) / intr[0] * d, (v - intr[3]) / intr[1] * d, d, np.ones_like(d)], -1).reshape(-1, 4)
        rows.append((cam @ est[k].T)[:, :3].astype(F32))
        origins.append(np.full(width * height, k, np.int32))
    return np.concatenate(rows), np.concatenate(origins), true, est, depths, intr, K


# frame 7 of the room loop against the rows of frames 0 .. 6 (rho = 0.05): rows tested / in front per frame, from the
# drifted pose of frame 7 and from its true pose, and the rows that agree (from the true pose some rows of the drifted
# frames 5 and 6 lie behind what frame 7 sees)
ROOM_TESTED = {"drifted": [19200, 19200, 19139, 18900, 17817, 17176, 17662],
               "true": [19080, 19080, 19024, 18859, 18649, 18092, 18340]}
ROOM_FRONT = {"drifted": [657, 171, 0, 0, 0, 0, 0], "true": [0, 0, 0, 0, 0, 0, 0]}
ROOM_AGREE = {"drifted": [18543, 19029, 19139, 18900, 17817, 17176, 17662],
              "true": [19080, 19080, 19024, 18859, 18649, 18065, 17991]}
