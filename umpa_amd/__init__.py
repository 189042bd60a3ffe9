"""
umpa_amd -- MI355X (gfx950) implementation of the UMPA per-pixel matching path.

Drop-in for the hot path of optimato/UMPA: ``match`` / ``match_unbiased`` and the
``UMPAModelNoDF`` / ``UMPAModelDF`` model classes keep the reference's API
(reference ``UMPA/__init__.py:8``, ``UMPA/speckle_matching.py``, ``UMPA/model.pyx``);
the numerics run in ``libumpa_hip.so`` (C ABI: ``include/umpa_hip.h``).  ``align`` holds the three
callers of ``UMPA/align.py`` that wrap the match (``UMPA_normal``, ``UMPA_nobias``, ``correct_bad_pixels``).
``UnwarpMap`` (``umpa_amd.unwarp``) is the detector distortion correction of the reference's batch script.
``umpa_amd.register`` holds the registration utilities of ``UMPA/align.py`` (``get_diff_pos``, ``get_new_sam_pos``,
``shift_data`` ...) on ``libumpa_register.so``; ``align`` re-exports them.
``integrate`` / ``phase_from_match`` (``umpa_amd.integrate``) turn the differential maps ``dx``, ``dy`` into the phase by a
weighted least-squares integration on ``libumpa_integrate.so``.
``KernelSearch`` (``umpa_amd.ddf``) finds the blur kernel ``(a, b, c)`` of the kernel dark-field model among candidates, per
pixel, on ``libumpa_ddf.so``: the directional dark-field signal.
``match_smooth`` / ``aggregate`` (``umpa_amd.smooth``) regularise the integer shift field by path aggregation over the cost
volume on ``libumpa_smooth.so`` and start the ordinary walk from it.
``uncertainty`` (``umpa_amd.sigma``) gives the per-pixel standard deviations of ``dx``, ``dy`` and a noise estimate, on
``libumpa_sigma.so``; ``Uncertainty.weight()`` feeds ``phase_from_match``.
``model.basins()`` gives, per pixel, the K lowest local minima of the cost over the search box, on ``libumpa_grid.so``;
``umpa_amd.basins`` holds the helpers that pick among them (``nearest``, ``select``, ``start_shifts``, ``ambiguity``).
``model.track()`` makes that choice on the device, among all basins, from a per-pixel prior; ``Tracker`` / ``prior_from``
(``umpa_amd.track``) run a step series on it, each projection's shifts being the next one's prior.
``widen=b`` on ``match(search='grid')``, ``cost_volume``, ``basins`` and ``track`` searches under a window ``b`` pixels wider,
on the same model; ``umpa_amd.widen`` has that window, the region of a widened result and ``coarse_to_fine``.
``scale_space`` (``umpa_amd.levels``) runs every widening level of that chain from one pass over the shift table and picks,
per pixel, the narrowest level that agrees with every wider one; ``select_levels`` states the rule in numpy.
``model.sequence()`` carries a per-pixel cost state through a series of projections (forward dynamic programming over the
shift table), so that one bad projection does not lock a wrong basin in; ``Sequence`` (``umpa_amd.sequence``) runs a step
series on it with the state on the device, ``restate`` states the rule in numpy.
"""
from . import model
from . import align
from . import register
from .model import UMPAModelNoDF, UMPAModelDF, UMPAModelDFKernel
from .speckle_matching import match, match_unbiased
from .unwarp import UnwarpMap
from .integrate import integrate, vcycle, phase_from_match, Integration
from . import ddf
from .ddf import (KernelSearch, gaussian_kernel, kernel_from_sigma, sigma_from_kernel, candidate_grid, blur_frames)
from . import smooth
from .smooth import aggregate, cost_scale, match_smooth
from . import sigma
from .sigma import uncertainty, Uncertainty
from . import basins
from . import track
from .track import Tracker, prior_from
from . import widen
from . import levels
from .levels import scale_space, select_levels
from . import sequence
from .sequence import Sequence, restate

__all__ = ["model", "align", "match", "match_unbiased", "UMPAModelNoDF", "UMPAModelDF", "UMPAModelDFKernel",
           "UnwarpMap", "integrate", "vcycle", "phase_from_match", "Integration",
           "ddf", "KernelSearch", "gaussian_kernel", "kernel_from_sigma", "sigma_from_kernel", "candidate_grid", "blur_frames",
           "smooth", "aggregate", "cost_scale", "match_smooth",
           "sigma", "uncertainty", "Uncertainty",
           "basins",
           "track", "Tracker", "prior_from",
           "widen",
           "levels", "scale_space", "select_levels",
           "sequence", "Sequence", "restate"]
