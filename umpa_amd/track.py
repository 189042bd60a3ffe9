"""
umpa_amd.track -- a step series on ``model.track()``.

``model.track(prior_dx, prior_dy, ...)`` (``include/umpa_grid.h``: ``umpa_grid_track``) picks, per pixel, the basin of the cost
that a prior shift selects.  In a step scan the natural prior of a projection is the result of the one before it:

  ``prior_from(result)``  ``(prior_dx, prior_dy)`` of a result dictionary: its ``dx``, ``dy`` with NaN where the match failed
                          (``err != 1``) or a map is not finite -- a NaN prior leaves the pixel to the data term;
  ``Tracker(model, lam=None, radius=None)``  ``.step(raw_frames, dark=None, flat=None)`` uploads the next sample stack
                          (``model.stage_sample``) and tracks it with the previous step's ``prior_from`` as the prior.  The
                          prior stays on the device between steps, and the maps of a step are HIP tensors.  The first step,
                          and the first after ``.reset()``, has an all-NaN prior: it is the grid search.
"""
import numpy as np

__all__ = ["Tracker", "prior_from"]


def prior_from(result):
    """``(prior_dx, prior_dy)`` for ``model.track()`` from a result of ``match()`` or ``track()``: numpy arrays or HIP tensors,
    as the result's maps are."""
    dx, dy, err = result["dx"], result["dy"], result["err"]
    if hasattr(dx, "data_ptr"):
        import torch
        ok = (err == 1) & torch.isfinite(dx) & torch.isfinite(dy)
        nan = torch.full_like(dx, float("nan"))
        return torch.where(ok, dx, nan), torch.where(ok, dy, nan)
    dx, dy = np.asarray(dx, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    ok = (np.asarray(err) == 1) & np.isfinite(dx) & np.isfinite(dy)
    return np.where(ok, dx, np.nan), np.where(ok, dy, np.nan)


class Tracker:
    """A step series on one model: every ``step`` is tracked with the previous step's shifts as its prior."""

    def __init__(self, model, lam=None, radius=None):
        if not hasattr(model, "track"):
            raise RuntimeError("Tracker needs a model with track() (UMPAModelNoDF or UMPAModelDF)")
        self.model, self.lam, self.radius = model, lam, radius
        self._prior = None

    def reset(self):
        """Forget the prior: the next step is the grid search again."""
        self._prior = None

    @property
    def prior(self):
        """``(prior_dx, prior_dy)`` the next step will use (HIP tensors), or None before the first step and after ``reset()``"""
        return self._prior

    def step(self, raw_frames, dark=None, flat=None):
        """Upload ``raw_frames`` as ``model.stage_sample`` takes them and track them over the model's ROI.  Returns the
        dictionary of ``model.track()``, its maps HIP tensors on the model's device."""
        import torch
        self.model.stage_sample(raw_frames, dark=dark, flat=flat)
        prior = self._prior
        if prior is None:
            d = self.model._device                                  # a model's is the index of its HIP device
            nan = torch.full(tuple(self.model.sh), float("nan"), dtype=torch.float64,
                             device=torch.device("cuda", d) if isinstance(d, int) else torch.device(d))
            prior = (nan, nan)
        result = self.model.track(prior[0], prior[1], lam=self.lam, radius=self.radius)
        self._prior = prior_from(result)
        return result
