"""
umpa_amd.sequence -- a step series on ``model.sequence()``.

``model.sequence(state, lam, trunc)`` (``include/umpa_grid.h``: ``umpa_grid_sequence``) is one forward step of a dynamic
programme over the projections of a step scan: per pixel an accumulated cost for every shift of the search box comes in,
this projection's costs are added to the cheapest compatible predecessor, and the new state goes out.  Unlike ``Tracker``,
whose prior is the one shift the previous projection chose, the state keeps every alternative alive: a projection that
picked a wrong basin does not decide the next one.

  ``Sequence(model, lam, trunc=None)``  ``.step(raw_frames, dark=None, flat=None)`` uploads the next sample stack
                          (``model.stage_sample``) and advances the state over the model's ROI.  The state stays on the
                          device between steps, in two tensors that take turns (none is allocated per step), and the maps
                          of a step are HIP tensors.  The first step, and the first after ``.reset()``, starts a series: it
                          is the grid search.
  ``restate(cost_volume, prev, lam, trunc)``  the definition in numpy, on a cost volume: what the library computes from
                          its own costs, expression for expression.
"""
import numpy as np

__all__ = ["Sequence", "restate"]


def _first_min(a, axis):
    """The value of the first strict minimum along ``axis``, starting at +Inf: NaN and +Inf never win (+Inf where none does)."""
    return np.where(a < np.inf, a, np.inf).min(axis=axis)


def restate(cost_volume, prev, lam, trunc=None):
    """The rule of ``umpa_grid_sequence`` on a cost volume ``[U, U, ...]`` (``cost_volume()['cost']``: row shift, column shift,
    then the pixels) and a previous state of the same shape (or ``None``); ``trunc=None`` is ``+Inf``.  Every operation is
    numpy's elementwise fp64 arithmetic, which rounds each product and each sum like the kernel.  Returns a dictionary of
    ``M`` (the transition term), ``state`` (``A = C + M``, the next state), ``index`` (the first strict minimum of ``A`` in scan
    order as ``si_index * U + sj_index``, -1 where no ``A`` is below +Inf), ``shift`` (int32 ``[2, ...]``, row shift first, zero
    at -1), ``cost`` (``C`` there), ``total`` (``A`` there), ``cost0`` (the first strict minimum of ``C``, 0 where none) and
    ``moved`` (int32)."""
    C = np.asarray(cost_volume, dtype=np.float64)
    U = C.shape[0]
    ms = (U + 1) // 2
    if C.ndim < 2 or C.shape[1] != U or U != 2 * ms - 1:
        raise ValueError("restate: the volume must be [U, U, ...] with U odd")
    lam = np.float64(lam)
    trunc = np.float64(np.inf if trunc is None else trunc)
    pix = C.shape[2:]
    M = np.zeros(C.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        if prev is not None:
            P = np.asarray(prev, dtype=np.float64)
            if P.shape != C.shape:
                raise ValueError("restate: the state must have the volume's shape")
            m0 = _first_min(P.reshape((U * U,) + pix), 0)
            pen = lam * (np.arange(U) ** 2).astype(np.float64)                       # lam * (double)(d * d)
            penm = pen[np.abs(np.arange(U)[:, None] - np.arange(U)[None, :])]          # [to, from]
            tail = (1,) * len(pix)
            R = np.empty(P.shape)
            for sj in range(U):                                                      # stage 2: along the columns of a row
                R[:, sj] = _first_min(P + penm[sj].reshape((1, U) + tail), 1)
            Q = np.empty(P.shape)
            for si in range(U):                                                      # stage 3: along the rows
                Q[si] = _first_min(R + penm[si].reshape((U, 1) + tail), 0)
            cap = m0 + trunc
            Q = np.where(cap[None, None] < Q, cap[None, None], Q)
            M = np.where((m0 < np.inf)[None, None], Q - m0[None, None], 0.0)
        A = C + M
        flatA, flatC = A.reshape((U * U,) + pix), C.reshape((U * U,) + pix)
        keyA, keyC = np.where(flatA < np.inf, flatA, np.inf), np.where(flatC < np.inf, flatC, np.inf)
        ia, ic = np.argmin(keyA, axis=0), np.argmin(keyC, axis=0)                     # the first of equal minima
        found, any_c = keyA.min(axis=0) < np.inf, keyC.min(axis=0) < np.inf
        take = lambda v, q: np.take_along_axis(v, q[None], axis=0)[0]
        out = {"M": M, "state": A, "index": np.where(found, ia, -1)}
        out["shift"] = np.stack([np.where(found, ia // U - (ms - 1), 0), np.where(found, ia % U - (ms - 1), 0)]).astype(np.int32)
        out["cost"] = np.where(found, take(flatC, ia), 0.0)
        out["total"] = np.where(found, take(flatA, ia), 0.0)
        out["cost0"] = np.where(any_c, take(flatC, ic), 0.0)
        out["moved"] = (found & (ia != ic)).astype(np.int32)
    return out


class Sequence:
    """A step series on one model: every ``step`` advances a per-pixel cost state kept on the device."""

    def __init__(self, model, lam, trunc=None):
        if not hasattr(model, "sequence"):
            raise RuntimeError("Sequence needs a model with sequence() (UMPAModelNoDF or UMPAModelDF)")
        self.model, self.lam, self.trunc = model, lam, trunc
        self._buffers, self._state = None, None

    def reset(self):
        """Forget the state: the next step starts a series (the grid search).  The two tensors are kept."""
        self._state = None

    @property
    def state(self):
        """The state the next step will read (a HIP tensor ``[U, U, N0, N1]``), or None before the first step and after
        ``reset()``"""
        return self._state

    def step(self, raw_frames, dark=None, flat=None):
        """Upload ``raw_frames`` as ``model.stage_sample`` takes them and advance the state over the model's ROI.  Returns the
        dictionary of ``model.sequence()``, its maps HIP tensors on the model's device; its ``state`` is valid until the step
        after the next one overwrites it."""
        import torch
        self.model.stage_sample(raw_frames, dark=dark, flat=flat)
        U = 2 * self.model.max_shift - 1
        shape = (U, U) + tuple(self.model.sh)
        if self._buffers is None or tuple(self._buffers[0].shape) != shape:
            d = self.model._device                                  # a model's is the index of its HIP device
            dev = torch.device("cuda", d) if isinstance(d, int) else torch.device(d)
            self._buffers = [torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(2)]
            self._state = None
        out = self._buffers[1] if self._state is self._buffers[0] else self._buffers[0]
        result = self.model.sequence(state=self._state, lam=self.lam, trunc=self.trunc, out=out)
        self._state = result["state"]
        return result
