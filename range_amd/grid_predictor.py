"""Dense predictions of a CSP class head on a lon/lat grid (reference: location_models/csp/main/
grid_predictor.py, the branch of the ``spa_enc`` encoders: (lon, lat) degrees, no date features).

``GridPredictor(mask, loc_model)``: ``mask`` (H, W), rows from latitude 90 down to -90, columns from longitude
-180 to 180; ``loc_model``: ``model.loc_model`` of ``load_model('CSP' | 'CSP_INat', ..., class_head=True)`` - or
anything with its ``forward(coords, class_of_interest=None, return_feats=True)`` and ``class_sum(coords)``.
The grid is built as the reference builds it, with CPU torch in float32 (``linspace(-1, 1, W) * 180``,
``linspace(1, -1, H) * 90``), and widened exactly to float64, as the reference's ``astype(float)`` does.  The
reference predicts column by column; here the grid goes through the model in row-major chunks of at most 2^18
locations (every location's result is independent of its batch, bit for bit)."""
from __future__ import annotations

import numpy as np
import torch

CHUNK = 1 << 18


def grid_coords(height: int, width: int) -> np.ndarray:
    """(H, W, 2) float64 (lon, lat) degrees of the reference's grid."""
    lon = (torch.linspace(-1, 1, width) * 180).numpy().astype(np.float64)
    lat = (torch.linspace(1, -1, height) * 90).numpy().astype(np.float64)
    out = np.empty((height, width, 2), dtype=np.float64)
    out[:, :, 0] = lon[None, :]
    out[:, :, 1] = lat[:, None]
    return out


def mask_lines(mask: np.ndarray) -> np.ndarray:
    """1 where the mask changes (grid_predictor.py:30-31), else 0."""
    g = np.gradient(mask)
    lines = g[0] ** 2 + g[1] ** 2
    lines[lines > 0.0] = 1.0
    return lines


class GridPredictor:
    def __init__(self, mask, loc_model, mask_only_pred: bool = False):
        self.mask = np.asarray(mask)
        if self.mask.ndim != 2:
            raise ValueError(f"mask must be (H, W), got {self.mask.shape}")
        self.loc_model = loc_model
        self.mask_lines = mask_lines(self.mask)
        self.feats = grid_coords(*self.mask.shape)
        if mask_only_pred:
            self.mask_inds = np.where(self.mask.ravel() == 1)[0]
            self.feats_local = self.feats.reshape(-1, 2)[self.mask_inds, :].copy()

    def _predict(self, coords: np.ndarray, fn) -> np.ndarray:
        """``fn`` (a (n,2) float64 tensor -> a (n,) float32 tensor) over ``coords`` (N,2) in chunks -> (N,) float32."""
        out = np.zeros((coords.shape[0],), dtype=np.float32)
        for i in range(0, coords.shape[0], CHUNK):
            r = fn(torch.from_numpy(np.ascontiguousarray(coords[i:i + CHUNK])))
            out[i:i + CHUNK] = r.cpu().numpy() if torch.is_tensor(r) else np.asarray(r, dtype=np.float32)
        return out

    def _apply_mask(self, grid_pred, mask_op: bool):
        return grid_pred * self.mask + self.mask_lines if mask_op else grid_pred

    def dense_prediction(self, class_of_interest, mask_op: bool = True) -> np.ndarray:
        """The probability of ``class_of_interest`` at every grid point, (H, W); ``mask_op``: times the mask, plus
        its outlines."""
        c = int(class_of_interest)
        pred = self._predict(self.feats.reshape(-1, 2),
                             lambda x: self.loc_model(x, class_of_interest=c, return_feats=False))
        return self._apply_mask(pred.reshape(self.mask.shape), mask_op)

    def dense_prediction_sum(self, mask_op: bool = True):
        """-> (the sum of all classes' probabilities at every grid point (H, W), its maximum before masking)."""
        pred = self._predict(self.feats.reshape(-1, 2), self.loc_model.class_sum).reshape(self.mask.shape)
        max_val = pred.max()
        return self._apply_mask(pred, mask_op), max_val

    def dense_prediction_masked(self, class_of_interest) -> np.ndarray:
        """Predictions at the mask's ones only (``mask_only_pred=True``), scattered into a zero (H, W) grid."""
        if not hasattr(self, "mask_inds"):
            raise ValueError("dense_prediction_masked needs GridPredictor(..., mask_only_pred=True)")
        c = int(class_of_interest)
        grid = np.zeros(self.mask.size, dtype=np.float32)
        if len(self.mask_inds):
            grid[self.mask_inds] = self._predict(self.feats_local,
                                                 lambda x: self.loc_model(x, class_of_interest=c, return_feats=False))
        return grid.reshape(self.mask.shape)
