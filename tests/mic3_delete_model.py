"""NumPy model of the 3-D fence-off deletion (plain helper module, no fixtures): the rule include/pylamp_hip.h gives at
pl3_mic_set_deletion, the extension of pylamp2.py:563-581 by one axis.

  * a tracer is outside when, for any axis d, x_d <= 0 or x_d >= L_d with L_d the last node coordinate (a NaN coordinate compares
    false: the tracer is kept);
  * the sort that removes it is, for everything else, the plain sort (+ census + refill) of the survivors alone: the deletion
    model is tests/mic3_refill_model.refill (tests/mic3_rect_model.refill with the per-axis search) applied to the kept rows.

With ONE cell layer along y and a y-invariant set the survivors are those of oracle.fence_and_delete(..., fence_enabled=False)
(tests/test_mic3_delete_model.py).
"""
import numpy as np

import mic3_rect_model as S
import mic3_refill_model as R


def outside(tr_x, L):
    """Mask of the tracers the next sort removes; L = the last node coordinate per axis."""
    tr_x = np.asarray(tr_x, dtype=np.float64)
    out = np.zeros(tr_x.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for d in range(3):
            out |= (tr_x[:, d] <= 0) | (tr_x[:, d] >= L[d])
    return out


def sort_delete_refill(tr_x, tr_f, grid, tracdens=0, tracdens_min=0, seed=0, it=0, unique_ids=False, tr_v=None, search=False):
    """(x, f, v, info, kept): the state a deleting sort leaves and the mask of the rows it kept.  info is that of refill() on the
    kept rows (counts, census and the largest ID are those of the survivors) with nremoved added."""
    tr_x = np.asarray(tr_x, dtype=np.float64); tr_f = np.asarray(tr_f, dtype=np.float64)
    kept = ~outside(tr_x, [np.asarray(g, dtype=np.float64)[-1] for g in grid])
    v = None if tr_v is None else np.asarray(tr_v, dtype=np.float64)[kept]
    refill = S.refill if search else R.refill
    x, f, v, info = refill(tr_x[kept], tr_f[kept], grid, tracdens, tracdens_min, seed, it, unique_ids=unique_ids, tr_v=v)
    info["nremoved"] = int((~kept).sum())
    return x, f, v, info, kept
