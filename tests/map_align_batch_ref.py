"""numpy mirror of csrc/map_align_batch.hip, on top of tests/map_align_ref.py (imported, not copied): every pose of a
batch is aligned as tests/map_align_ref.pose_align aligns it alone -- the batch kernel promises those bits -- and what
the batch adds is worked out from the history: the three-valued ``done`` word, and which sums the call leaves.

  done = 0  every iteration STEPPED;
  done = 1  the first status that is not STEPPED is CONVERGED, at the last iteration: the closing pass never ran, and the
            sums are those of the pose before that step;
  done = 2  CONVERGED earlier (the next iteration took the sums at the final pose and closed the pose), or FEW, SINGULAR,
            TOO_FAR at any iteration (the pose did not move: the sums are at the final pose already).

pose_align recomputes the sums whenever the pose has moved and returns the last ones it computed, which in each of the
three cases are the sums the device leaves."""
import numpy as np

from tests import map_align_ref as ref


def done_of(rows):
    """The batch's done word from the history's integers [steps,4] of one pose."""
    status = rows[:, 0].tolist()
    moving = [k for k, s in enumerate(status) if s != ref.STEPPED]
    if not moving:
        return 0
    first = moving[0]
    return 1 if status[first] == ref.CONVERGED and first == len(status) - 1 else 2


def pose_align_batch(means, w2cs, intr, depth, keep, beyond, kappa, near, max_steps, damping, min_used, max_rot, max_trans,
                     eps_rot, eps_trans):
    """Per pose of w2cs [k,4,4]: (P [3,4] float64, work [4,4] float32, steps_taken, done in 0 .. 2, rows [max_steps,4]
    int64, xis [max_steps,6] float64, sums [30] int64) -- what gsl_map_pose_align_batch leaves for it."""
    out = []
    for w2c in np.asarray(w2cs, dtype=np.float32).reshape(-1, 4, 4):
        P, work, taken, _, rows, xis, sums = ref.pose_align(means, w2c, intr, depth, keep, beyond, kappa, near, max_steps,
                                                            damping, min_used, max_rot, max_trans, eps_rot, eps_trans)
        out.append((P, work, taken, done_of(rows), rows, xis, np.asarray(sums, dtype=np.int64)))
    return out
