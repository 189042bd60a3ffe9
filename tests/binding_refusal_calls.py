"""
The calls that the Python bindings (``umpa_amd/*.py``) refuse themselves, one row per ``raise`` that an argument can reach in
the entry points that take "host arrays or HIP tensors" (``sigma.region`` / ``solve``, ``smooth.aggregate``,
``register.shift_sums``, ``integrate.integrate`` / ``rhs`` / ``vcycle``, ``ddf.blur_frames`` / ``fold``), in the region
resolution of the models and of ``ddf.KernelSearch``, and in the models' ``cost_volume`` / ``match_smooth`` / ``uncertainty``
fronts; per function at least one call that breaks two rules at once (which of them answers is part of the contract).
tests/golden/make_golden_binding_refusals.py records the exception type and the complete text of every row into
tests/golden/binding_refusals_observed.json; tests/test_binding_refusals.py replays the rows and compares both exactly.

A row is ``(id, needs, call, no_device)``.  ``needs`` is ``"host"`` (numpy arrays only: replayed without a GPU) or
``"device"`` (HIP tensors or a model: replayed on the GPU); ``call(c)`` makes the call with the context ``c`` (``Context``
below; host rows do not touch it); ``no_device`` rows pass every check of the binding and are answered by the library's
device count, so they hold only where there is no HIP device.

Shapes: stacks ``[2, 20, 22]`` with a 5 x 5 window and ``max_shift=3`` (extent 10 x 12), cost volumes ``[3, 3, 4, 5]``,
maps of 8 x 9, ddf frames of 17 x 17.  The kernel dark-field model and ``KernelSearch`` pad by 8 pixels more and do not
exist on 20 x 22 frames: their rows use ``[2, 30, 32]`` with a 3 x 3 window and ``max_shift=2`` (extent 8 x 10).
"""
import numpy as np

# (``umpa_amd.integrate`` and ``umpa_amd.register`` name functions of the package: the modules are imported by their path)
NAN, INF = float("nan"), float("inf")


def _stack(K, H, W, seed=0):
    return 1.0 + np.random.default_rng(seed).random((K, H, W))


class Context:
    """What the device rows share: ``dev`` (a numpy array as a contiguous HIP tensor), ``strided`` (the same values as a
    non-contiguous one) and the models, each built at first use."""

    def __init__(self):
        self._models = {}

    @staticmethod
    def dev(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    @classmethod
    def strided(cls, a):
        a = np.asarray(a)
        return cls.dev(np.repeat(a, 2, axis=-1))[..., ::2]

    def model(self, name):
        if name not in self._models:
            from umpa_amd import ddf, model as M
            sam, ref = _stack(2, 20, 22, 1), _stack(2, 20, 22, 2)
            big_s, big_r = _stack(2, 30, 32, 3), _stack(2, 30, 32, 4)
            kw = dict(window_size=2, max_shift=3)
            if name == "plain":
                m = M.UMPAModelNoDF(list(sam), list(ref), **kw)
            elif name == "df":
                m = M.UMPAModelDF(list(sam), list(ref), **kw)
            elif name == "masked":
                m = M.UMPAModelNoDF(list(sam), list(ref), mask_list=list(np.ones_like(sam)), **kw)
            elif name == "stepped":
                m = M.UMPAModelNoDF(list(sam), list(ref), pos_list=[(0, 0), (1, 2)], **kw)
            elif name == "ref_coordinates":
                m = M.UMPAModelNoDF(list(sam), list(ref), **kw)
                m.assign_coordinates = 'ref'
            elif name == "narrow":
                m = M.UMPAModelNoDF(list(sam), list(ref), window_size=2, max_shift=1)
            elif name == "staged":
                m = M.UMPAModelNoDF(list(sam), list(ref), **kw)
                m.stage_sample(list(sam))
            elif name == "kernel":
                m = M.UMPAModelDFKernel(list(big_s), list(big_r), window_size=1, max_shift=2)
            elif name == "search":
                m = ddf.KernelSearch(list(big_s), list(big_r), window_size=1, max_shift=2)
            m.debug = False
            self._models[name] = m
        if name != "search":
            self._models[name].ROI = None                             # no row sees the region another one left behind
        return self._models[name]

    def result(self):
        """``plain.match()`` on the whole extent (the model's ROI is left there)."""
        if "result" not in self._models:
            self._models["result"] = self.model("plain").match(quiet=True)
        return self._models["result"]


def rows():
    from importlib import import_module
    ddf, integrate, register, sigma, smooth, M = (import_module("umpa_amd." + name) for name in ("ddf", "integrate", "register", "sigma", "smooth", "model"))
    out = []

    def row(name, call, needs="host", no_device=False):
        out.append((name, needs, call, no_device))

    def host(prefix, cases):
        for name, call in cases:
            row(prefix + ":" + name, call)

    def device(prefix, cases):
        for name, call in cases:
            row(prefix + ":device:" + name, call, "device")

    # ------------------------------------------------------------------ sigma.region
    sam, win, shift = _stack(2, 20, 22), np.full((5, 5), 1.0 / 25), np.zeros((2, 3, 4), dtype=np.int32)
    reg = (0, 1, 3, 0, 1, 4)

    def region(c=None, a=sam, b=sam, w=win, kind=0, area=reg, s=shift, wrap=lambda x: x, **kw):
        return sigma.region(wrap(a), wrap(b), w, 3, kind, area, wrap(s), **kw)

    host("sigma.region", [
        ("kind_2", lambda c: region(kind=2)), ("win_even", lambda c: region(w=np.ones((4, 4)) / 16)),
        ("win_not_square", lambda c: region(w=np.ones((3, 5)) / 15)), ("win_1d", lambda c: region(w=np.ones(5) / 5)),
        ("empty_rows", lambda c: region(area=(0, 1, 0, 0, 1, 4))), ("empty_columns", lambda c: region(area=(0, 1, 3, 0, 1, -1))),
        ("stack_2d", lambda c: region(a=sam[0], b=sam[0])), ("stacks_differ", lambda c: region(b=sam[:, :-1])),
        ("shift_shape", lambda c: region(s=shift[:, :2])), ("shift_planes", lambda c: region(s=shift[:1])),
        ("kind+win", lambda c: region(kind=-1, w=np.ones((4, 4)))), ("win+empty", lambda c: region(w=np.ones((2, 2)), area=(0, 1, 0, 0, 1, 4))),
        ("empty+stacks", lambda c: region(area=(0, 1, 3, 0, 1, 0), b=sam[:1])), ("stacks+shift", lambda c: region(b=sam[:, :, :-1], s=shift[:, :2])),
    ])
    row("sigma.region:no_device", lambda c: region(), no_device=True)
    row("sigma.region:no_device+float32_is_converted", lambda c: region(a=sam.astype(np.float32), s=shift.astype(np.int64)), no_device=True)
    device("sigma.region", [
        ("mixed_ref", lambda c: sigma.region(c.dev(sam), sam, win, 3, 0, reg, c.dev(shift))),
        ("mixed_shift", lambda c: sigma.region(c.dev(sam), c.dev(sam), win, 3, 0, reg, shift)),
        ("mixed_sam", lambda c: sigma.region(sam, c.dev(sam), win, 3, 0, reg, c.dev(shift))),
        ("sam_float32", lambda c: region(a=sam.astype(np.float32), wrap=c.dev)), ("shift_int64", lambda c: region(s=shift.astype(np.int64), wrap=c.dev)),
        ("stacks_differ", lambda c: region(b=sam[:, :-1], wrap=c.dev)), ("shift_shape", lambda c: region(s=shift[:, :2], wrap=c.dev)),
        ("not_contiguous", lambda c: sigma.region(c.strided(sam), c.dev(sam), win, 3, 0, reg, c.dev(shift))),
        ("shift_not_contiguous", lambda c: sigma.region(c.dev(sam), c.dev(sam), win, 3, 0, reg, c.strided(shift))),
        ("empty+mixed", lambda c: sigma.region(c.dev(sam), sam, win, 3, 0, (0, 1, 0, 0, 1, 4), c.dev(shift))),
        ("mixed+dtype", lambda c: sigma.region(c.dev(sam.astype(np.float32)), sam, win, 3, 0, reg, c.dev(shift))),
        ("dtype+stacks", lambda c: region(a=sam.astype(np.float32), b=sam[:, :-1].astype(np.float32), wrap=c.dev)),
        ("shift_shape+not_contiguous", lambda c: sigma.region(c.strided(sam), c.dev(sam), win, 3, 0, reg, c.dev(shift[:, :2]))),
    ])

    # ------------------------------------------------------------------ sigma.solve
    mom = np.ones((16, 4, 5))
    host("sigma.solve", [
        ("kind_3", lambda c: sigma.solve(mom, 3, 2, 0.1)), ("planes_of_the_other_kind", lambda c: sigma.solve(mom, 1, 2, 0.1)),
        ("one_dimension", lambda c: sigma.solve(np.ones(16), 0, 2, 0.1)), ("no_pixel", lambda c: sigma.solve(np.ones((16, 0, 5)), 0, 2, 0.1)),
        ("kind+planes", lambda c: sigma.solve(np.ones((3, 4)), 2, 2, 0.1)), ("planes+no_pixel", lambda c: sigma.solve(np.ones((34, 0)), 0, 2, 0.1)),
    ])
    row("sigma.solve:no_device", lambda c: sigma.solve(mom, 0, 2, 0.1), no_device=True)
    device("sigma.solve", [
        ("float32", lambda c: sigma.solve(c.dev(mom.astype(np.float32)), 0, 2, 0.1)), ("not_contiguous", lambda c: sigma.solve(c.strided(mom), 0, 2, 0.1)),
        ("planes+dtype", lambda c: sigma.solve(c.dev(np.ones((34, 4), dtype=np.float32)), 0, 2, 0.1)),
        ("no_pixel+dtype", lambda c: sigma.solve(c.dev(np.ones((16, 0), dtype=np.float32)), 0, 2, 0.1)),
        ("dtype+not_contiguous", lambda c: sigma.solve(c.strided(mom.astype(np.float32)), 0, 2, 0.1)),
    ])

    # ------------------------------------------------------------------ smooth.aggregate
    vol = _stack(9, 4, 5).reshape(3, 3, 4, 5)
    host("smooth.aggregate", [
        ("lam_negative", lambda c: smooth.aggregate(vol, -1.0, 2.0)), ("lam_nan", lambda c: smooth.aggregate(vol, NAN, 2.0)),
        ("trunc_negative", lambda c: smooth.aggregate(vol, 1.0, -2.0)), ("paths_6", lambda c: smooth.aggregate(vol, 1.0, 2.0, paths=6)),
        ("dirs_0", lambda c: smooth.aggregate(vol, 1.0, 2.0, dirs=0)), ("dirs_256", lambda c: smooth.aggregate(vol, 1.0, 2.0, dirs=256)),
        ("cost_2d", lambda c: smooth.aggregate(vol[0, 0], 1.0, 2.0)), ("cost_not_square", lambda c: smooth.aggregate(vol[:2], 1.0, 2.0)),
        ("cost_flat_not_a_square", lambda c: smooth.aggregate(vol.reshape(9, 4, 5)[:8], 1.0, 2.0)),
        ("U_even", lambda c: smooth.aggregate(np.ones((4, 4, 4, 5)), 1.0, 2.0)), ("U_1", lambda c: smooth.aggregate(np.ones((1, 1, 4, 5)), 1.0, 2.0)),
        ("U_17", lambda c: smooth.aggregate(np.ones((17, 17, 1, 1)), 1.0, 2.0)), ("empty", lambda c: smooth.aggregate(np.ones((3, 3, 0, 5)), 1.0, 2.0)),
        ("lam+trunc", lambda c: smooth.aggregate(vol, -1.0, NAN)), ("trunc+paths", lambda c: smooth.aggregate(vol, 1.0, -1.0, paths=5)),
        ("paths+cost", lambda c: smooth.aggregate(vol[:2], 1.0, 2.0, paths=5)), ("dirs+cost", lambda c: smooth.aggregate(vol[:2], 1.0, 2.0, dirs=-1)),
        ("U_even+empty", lambda c: smooth.aggregate(np.ones((4, 4, 0, 5)), 1.0, 2.0)),
    ])
    row("smooth.aggregate:no_device", lambda c: smooth.aggregate(vol, 1.0, 2.0, return_total=True), no_device=True)
    row("smooth.aggregate:no_device+flat_float32", lambda c: smooth.aggregate(vol.reshape(9, 4, 5).astype(np.float32), 0.0, INF, paths=4), no_device=True)
    device("smooth.aggregate", [
        ("float32", lambda c: smooth.aggregate(c.dev(vol.astype(np.float32)), 1.0, 2.0)), ("not_contiguous", lambda c: smooth.aggregate(c.strided(vol), 1.0, 2.0)),
        ("U_even", lambda c: smooth.aggregate(c.dev(np.ones((4, 4, 4, 5))), 1.0, 2.0)),
        ("dtype+U_even", lambda c: smooth.aggregate(c.dev(np.ones((4, 4, 4, 5), dtype=np.float32)), 1.0, 2.0)),
        ("cost_shape+not_contiguous", lambda c: smooth.aggregate(c.strided(vol[:2]), 1.0, 2.0)),
        ("dirs+dtype", lambda c: smooth.aggregate(c.dev(vol.astype(np.float32)), 1.0, 2.0, dirs=0)),
    ])

    # ------------------------------------------------------------------ register.shift_sums
    fr = _stack(2, 8, 9)
    one = np.ones((2, 8, 9))

    def weights(value):
        w = one.copy()
        w[1, 2, 3] = value
        return w

    host("register.shift_sums", [
        ("boundary", lambda c: register.shift_sums(fr, fr, boundary="clamp")), ("max_shift_negative", lambda c: register.shift_sums(fr, fr, max_shift=-1)),
        ("max_shift_fraction", lambda c: register.shift_sums(fr, fr, max_shift=1.5)), ("max_shift_triple", lambda c: register.shift_sums(fr, fr, max_shift=(1, 1, 1))),
        ("max_shift_33", lambda c: register.shift_sums(fr, fr, max_shift=(1, 33))),
        ("int32_frames", lambda c: register.shift_sums(fr.astype(np.int32), fr.astype(np.int32), max_shift=1)),
        ("a_other_dtype", lambda c: register.shift_sums(fr.astype(np.float32), fr, max_shift=1)),
        ("b_4d", lambda c: register.shift_sums(fr, fr[None], max_shift=1)), ("a_other_frame", lambda c: register.shift_sums(fr[:, :-1], fr, max_shift=1)),
        ("a_stack_b_frame", lambda c: register.shift_sums(fr, fr[0], max_shift=1)), ("a_other_count", lambda c: register.shift_sums(fr[:1], fr, max_shift=1)),
        ("w_other_frame", lambda c: register.shift_sums(fr, fr, one[:, :, :-1], max_shift=1)), ("w_other_count", lambda c: register.shift_sums(fr, fr, one[:1], max_shift=1)),
        ("box_taller_than_frame", lambda c: register.shift_sums(fr, fr, max_shift=(4, 0))), ("box_wider_than_frame", lambda c: register.shift_sums(fr, fr, max_shift=(0, 5))),
        ("weight_nan", lambda c: register.shift_sums(fr, fr, weights(NAN), max_shift=1)), ("weight_negative", lambda c: register.shift_sums(fr, fr, weights(-1.0), max_shift=1)),
        ("weight_inf", lambda c: register.shift_sums(fr, fr, weights(INF), max_shift=1)),
        ("boundary+max_shift", lambda c: register.shift_sums(fr, fr, boundary="clamp", max_shift=-1)),
        ("max_shift+dtype", lambda c: register.shift_sums(fr.astype(np.int8), fr.astype(np.int8), max_shift=40)),
        ("dtype+shape", lambda c: register.shift_sums(fr[:, :-1].astype(np.float32), fr, max_shift=1)),
        ("a_shape+w_shape", lambda c: register.shift_sums(fr[:, :-1], fr, one[:1], max_shift=1)), ("w_shape+box", lambda c: register.shift_sums(fr, fr, one[:1], max_shift=5)),
        ("box+weight", lambda c: register.shift_sums(fr, fr, weights(NAN), max_shift=5)),
    ])
    row("register.shift_sums:no_device", lambda c: register.shift_sums(fr, fr, one[0], max_shift=1), no_device=True)
    row("register.shift_sums:no_device+uint16_shared_a", lambda c: register.shift_sums(fr[0].astype(np.uint16), fr.astype(np.uint16), max_shift=(1, 2), boundary="overlap"), no_device=True)
    device("register.shift_sums", [
        ("int32_frames", lambda c: register.shift_sums(c.dev(fr.astype(np.int32)), c.dev(fr.astype(np.int32)), max_shift=1)),
        ("a_other_dtype", lambda c: register.shift_sums(c.dev(fr.astype(np.float32)), c.dev(fr), max_shift=1)),
        ("w_float32", lambda c: register.shift_sums(c.dev(fr), c.dev(fr), c.dev(one.astype(np.float32)), max_shift=1)),
        ("a_on_the_host", lambda c: register.shift_sums(fr, c.dev(fr), max_shift=1)), ("w_on_the_host", lambda c: register.shift_sums(c.dev(fr), c.dev(fr), one, max_shift=1)),
        ("a_other_frame", lambda c: register.shift_sums(c.dev(fr[:, :-1]), c.dev(fr), max_shift=1)), ("w_other_count", lambda c: register.shift_sums(c.dev(fr), c.dev(fr), c.dev(one[:1]), max_shift=1)),
        ("box_wider_than_frame", lambda c: register.shift_sums(c.dev(fr), c.dev(fr), max_shift=(0, 5))),
        ("b_not_contiguous", lambda c: register.shift_sums(c.dev(fr), c.strided(fr), max_shift=1)), ("w_not_contiguous", lambda c: register.shift_sums(c.dev(fr), c.dev(fr), c.strided(one), max_shift=1)),
        ("dtype+shape", lambda c: register.shift_sums(c.dev(fr[:, :-1].astype(np.float32)), c.dev(fr), max_shift=1)),
        ("box+not_contiguous", lambda c: register.shift_sums(c.strided(fr), c.dev(fr), max_shift=5)),
        ("max_shift+dtype", lambda c: register.shift_sums(c.dev(fr.astype(np.int32)), c.dev(fr.astype(np.int32)), max_shift=33)),
    ])

    # ------------------------------------------------------------------ integrate.integrate / rhs
    g = _stack(2, 8, 9)

    def bad_weight(value, shape=(2, 8, 9)):
        w = np.ones(shape)
        w[(Ellipsis, 2, 3)] = value
        return w

    host("integrate.integrate", [
        ("tol_nan", lambda c: integrate.integrate(g, g, tol=NAN)), ("tol_negative", lambda c: integrate.integrate(g, g, tol=-1e-3)),
        ("maxiter_negative", lambda c: integrate.integrate(g, g, maxiter=-1)), ("maxiter_fraction", lambda c: integrate.integrate(g, g, maxiter=2.5)),
        ("gx_4d", lambda c: integrate.integrate(g[None], g[None])), ("gx_1d", lambda c: integrate.integrate(g[0, 0], g[0, 0])),
        ("gy_differs", lambda c: integrate.integrate(g, g[:, :-1])), ("weight_differs", lambda c: integrate.integrate(g, g, one[0])),
        ("one_row", lambda c: integrate.integrate(g[:, :1], g[:, :1])), ("one_column", lambda c: integrate.integrate(g[0, :, :1], g[0, :, :1])),
        ("weight_nan", lambda c: integrate.integrate(g, g, bad_weight(NAN))), ("weight_negative", lambda c: integrate.integrate(g, g, bad_weight(-0.5))),
        ("weight_inf", lambda c: integrate.integrate(g[0], g[0], bad_weight(INF, (8, 9)))),
        ("tol+maxiter", lambda c: integrate.integrate(g, g, tol=INF, maxiter=-1)), ("maxiter+gy", lambda c: integrate.integrate(g, g[0], maxiter=-1)),
        ("gy+weight_shape", lambda c: integrate.integrate(g, g[0], one[:1])), ("weight_shape+small", lambda c: integrate.integrate(g[:, :1], g[:, :1], one)),
        ("small+weight", lambda c: integrate.integrate(g[:, :1], g[:, :1], bad_weight(NAN)[:, :1])),
        ("rhs_gy_differs", lambda c: integrate.rhs(g, g[:, :-1])), ("rhs_weight_nan", lambda c: integrate.rhs(g, g, bad_weight(NAN))),
    ])
    row("integrate.integrate:no_device", lambda c: integrate.integrate(g, g, one), no_device=True)
    row("integrate.integrate:no_device+float32_single_map", lambda c: integrate.integrate(g[0].astype(np.float32), g[0], maxiter=0), no_device=True)
    device("integrate.integrate", [
        ("mixed_gy", lambda c: integrate.integrate(c.dev(g), g)), ("mixed_gx", lambda c: integrate.integrate(g, c.dev(g))),
        ("mixed_weight", lambda c: integrate.integrate(c.dev(g), c.dev(g), one)), ("mixed_weight_alone_on_the_device", lambda c: integrate.integrate(g, g, c.dev(one))),
        ("gy_differs", lambda c: integrate.integrate(c.dev(g), c.dev(g[:, :-1]))), ("weight_differs", lambda c: integrate.integrate(c.dev(g), c.dev(g), c.dev(one[0]))),
        ("one_row", lambda c: integrate.integrate(c.dev(g[:, :1]), c.dev(g[:, :1]))),
        ("gx_float32", lambda c: integrate.integrate(c.dev(g.astype(np.float32)), c.dev(g))), ("weight_float32", lambda c: integrate.integrate(c.dev(g), c.dev(g), c.dev(one.astype(np.float32)))),
        ("gy_not_contiguous", lambda c: integrate.integrate(c.dev(g), c.strided(g))), ("weight_not_contiguous", lambda c: integrate.integrate(c.dev(g), c.dev(g), c.strided(one))),
        ("tol+mixed", lambda c: integrate.integrate(c.dev(g), g, tol=-1.0)), ("mixed+shape", lambda c: integrate.integrate(c.dev(g), g[:, :-1])),
        ("shape+dtype", lambda c: integrate.integrate(c.dev(g.astype(np.float32)), c.dev(g[:, :-1]))),
        ("dtype+not_contiguous", lambda c: integrate.integrate(c.strided(g), c.dev(g.astype(np.float32)))),
        ("rhs_mixed", lambda c: integrate.rhs(c.dev(g), g)),
    ])

    # ------------------------------------------------------------------ integrate.vcycle
    r = _stack(1, 8, 9)[0]
    host("integrate.vcycle", [
        ("r_3d", lambda c: integrate.vcycle(g)), ("weight_differs", lambda c: integrate.vcycle(r, one[0, :, :-1])),
        ("weight_nan", lambda c: integrate.vcycle(r, bad_weight(NAN, (8, 9)))), ("weight_negative", lambda c: integrate.vcycle(r, bad_weight(-1.0, (8, 9)), jacobi=True)),
        ("r_3d+weight", lambda c: integrate.vcycle(g, bad_weight(NAN))), ("shape+weight", lambda c: integrate.vcycle(r, bad_weight(NAN, (8, 8)))),
    ])
    row("integrate.vcycle:no_device", lambda c: integrate.vcycle(r, one[0]), no_device=True)
    row("integrate.vcycle:no_device+diagonal_float32", lambda c: integrate.vcycle(r.astype(np.float32), diagonal=True, no_tail=True), no_device=True)
    device("integrate.vcycle", [
        ("mixed_weight", lambda c: integrate.vcycle(c.dev(r), one[0])), ("mixed_r", lambda c: integrate.vcycle(r, c.dev(one[0]))),
        ("r_3d", lambda c: integrate.vcycle(c.dev(g))), ("weight_differs", lambda c: integrate.vcycle(c.dev(r), c.dev(one[0, :, :-1]))),
        ("r_float32", lambda c: integrate.vcycle(c.dev(r.astype(np.float32)))), ("weight_float32", lambda c: integrate.vcycle(c.dev(r), c.dev(one[0].astype(np.float32)))),
        ("r_not_contiguous", lambda c: integrate.vcycle(c.strided(r))), ("weight_not_contiguous", lambda c: integrate.vcycle(c.dev(r), c.strided(one[0]))),
        ("mixed+shape", lambda c: integrate.vcycle(c.dev(g), one[0])), ("shape+dtype", lambda c: integrate.vcycle(c.dev(g.astype(np.float32)))),
        ("dtype+not_contiguous", lambda c: integrate.vcycle(c.strided(r.astype(np.float32)))),
    ])

    # ------------------------------------------------------------------ ddf.blur_frames
    f17 = _stack(2, 17, 17)
    abc = (0.1, 0.0, 0.1)
    host("ddf.blur_frames", [
        ("a_zero", lambda c: ddf.blur_frames(f17, (0.0, 0.0, 0.1))), ("indefinite", lambda c: ddf.blur_frames(f17, (1.0, 3.0, 1.0))),
        ("b_nan", lambda c: ddf.blur_frames(f17, (0.1, NAN, 0.1))), ("no_frames", lambda c: ddf.blur_frames([], abc)),
        ("unequal_shapes", lambda c: ddf.blur_frames([f17[0], _stack(1, 17, 18)[0]], abc)), ("frames_3d", lambda c: ddf.blur_frames([f17, f17], abc)),
        ("H_16", lambda c: ddf.blur_frames(f17[:, :16], abc)), ("W_16", lambda c: ddf.blur_frames(f17[0, :, :16], abc)),
        ("kernel+no_frames", lambda c: ddf.blur_frames([], (0.0, 0.0, 0.1))), ("unequal+small", lambda c: ddf.blur_frames([f17[0, :16], f17[1]], abc)),
        ("three_dimensions+small", lambda c: ddf.blur_frames([f17[:, :16]], abc)),
    ])
    row("ddf.blur_frames:no_device", lambda c: ddf.blur_frames(f17, abc), no_device=True)
    row("ddf.blur_frames:no_device+single_float32", lambda c: ddf.blur_frames(f17[0].astype(np.float32), abc), no_device=True)
    device("ddf.blur_frames", [
        ("float32", lambda c: ddf.blur_frames(c.dev(f17.astype(np.float32)), abc)), ("not_contiguous", lambda c: ddf.blur_frames(c.strided(f17), abc)),
        ("second_on_the_host", lambda c: ddf.blur_frames([c.dev(f17[0]), f17[1]], abc)), ("frames_3d", lambda c: ddf.blur_frames([c.dev(f17)], abc)),
        ("unequal_shapes", lambda c: ddf.blur_frames([c.dev(f17[0]), c.dev(_stack(1, 17, 18)[0])], abc)), ("H_16", lambda c: ddf.blur_frames(c.dev(f17[:, :16]), abc)),
        ("kernel+dtype", lambda c: ddf.blur_frames(c.dev(f17.astype(np.float32)), (0.1, 1.0, 0.1))), ("dtype+small", lambda c: ddf.blur_frames(c.dev(f17[:, :16].astype(np.float32)), abc)),
        ("not_contiguous+unequal", lambda c: ddf.blur_frames([c.strided(f17[0]), c.dev(f17[1, :16])], abc)),
    ])

    # ------------------------------------------------------------------ ddf.fold
    d4, e4 = np.zeros(6), np.zeros(6, dtype=np.int32)

    def fold(swap=None, m=0):
        planes = [d4, d4, d4, d4, e4, d4.copy(), d4.copy(), d4.copy(), d4.copy(), e4.copy(), e4.copy()]
        for k, v in (swap or {}).items():
            planes[k] = v
        return ddf.fold(m, planes[:5], planes[5:])

    host("ddf.fold", [
        ("f_float32", lambda c: fold({0: d4.astype(np.float32)})), ("err_float64", lambda c: fold({4: d4})), ("index_int64", lambda c: fold({9: e4.astype(np.int64)})),
        ("best_err_float64", lambda c: fold({10: d4})), ("dx_not_contiguous", lambda c: fold({2: np.zeros(12)[::2]})), ("best_T_other_size", lambda c: fold({6: np.zeros(5)})),
        ("dtype+size", lambda c: fold({1: np.zeros(5, dtype=np.float32)})), ("two_planes", lambda c: fold({3: np.zeros(12)[::2], 7: np.zeros(7)})),
    ])
    row("ddf.fold:no_device", lambda c: fold(), no_device=True)
    row("ddf.fold:no_device+2d_planes", lambda c: ddf.fold(1, [d4.reshape(2, 3)] * 4 + [e4.reshape(2, 3)], [d4.copy().reshape(2, 3) for _ in range(4)] + [e4.copy(), e4.copy()]), no_device=True)

    # ------------------------------------------------------------------ register.shift_data (the device default only; one refusal)
    host("register.shift_data", [
        ("frames_2d", lambda c: register.shift_data(fr[0], [(0, 0)])), ("shifts_of_another_count", lambda c: register.shift_data(fr, [(0, 0)])),
    ])

    # ------------------------------------------------------------------ the kernel model's uncertainty (unbound, as tests/test_sigma_cpu.py calls it)
    res34 = {"dx": np.zeros((3, 4)), "dy": np.zeros((3, 4)), "err": np.ones((3, 4), dtype=np.int32)}
    host("model.UMPAModelDFKernel.uncertainty", [("unbound", lambda c: M.UMPAModelDFKernel.uncertainty(None, res34))])

    # ------------------------------------------------------------------ the models: region resolution at every site
    empty, beyond, before, backwards = ((3, 3, 1), (0, 12, 1)), ((0, 11, 1), (0, 12, 1)), ((-1, 5, 1), (0, 12, 1)), ((0, 10, 1), (0, 12, -1))
    whole = ((0, 10, 1), (0, 12, 1))
    regions = [("steps_not_positive", dict(ROI=backwards)), ("step_zero_in_ROI", dict(ROI=((0, 10, 0), (0, 12, 1)))), ("empty", dict(ROI=empty)),
               ("beyond_the_extent", dict(ROI=beyond)), ("before_the_extent", dict(ROI=before)), ("columns_beyond", dict(ROI=((0, 10, 1), (4, 14, 3)))),
               ("step_negative", dict(step=-1)), ("steps+empty", dict(ROI=((3, 3, -1), (0, 12, 1)))), ("empty+beyond", dict(ROI=((3, 3, 1), (0, 13, 1)))),
               ("ROI_and_step", dict(ROI=empty, step=2))]
    sites = [("model.match", lambda c, kw: c.model("plain").match(quiet=True, **kw)), ("model.match_grid", lambda c, kw: c.model("df").match(quiet=True, search='grid', **kw)),
             ("model.coverage", lambda c, kw: c.model("plain").coverage(**kw)), ("model.cost_volume", lambda c, kw: c.model("plain").cost_volume(**kw)),
             ("smooth.match_smooth", lambda c, kw: smooth.match_smooth(c.model("plain"), **kw)),
             ("sigma.uncertainty", lambda c, kw: sigma.uncertainty(c.model("plain"), c.result(), **kw))]
    for site, fn in sites:
        for name, kw in regions:
            row("%s:region:%s" % (site, name), lambda c, fn=fn, kw=kw: fn(c, kw), "device")
    def remembered(c):
        m = c.model("df")
        m.match(quiet=True, ROI=whole)
        _refused(lambda: m.match(quiet=True, ROI=beyond))
        return m.match(quiet=True)                                    # match() stored the region before it refused it

    row("model.match:a_refused_ROI_is_remembered", remembered, "device")

    # ------------------------------------------------------------------ the models: what else they refuse around the region
    abc8 = np.tile(np.array([0.1, 0.0, 0.1]), (8, 10, 1))
    device("model.match", [
        ("search", lambda c: c.model("plain").match(quiet=True, search='spiral')), ("grid_dxdy", lambda c: c.model("plain").match(quiet=True, search='grid', dxdy=(0, 0))),
        ("grid_masked", lambda c: c.model("masked").match(quiet=True, search='grid')), ("grid_pos_list", lambda c: c.model("stepped").match(quiet=True, search='grid')),
        ("search+ROI", lambda c: c.model("plain").match(quiet=True, search='spiral', ROI=empty)), ("grid_masked+dxdy", lambda c: c.model("masked").match(quiet=True, search='grid', dxdy=(0, 0))),
        ("grid_dxdy+ROI", lambda c: c.model("plain").match(quiet=True, search='grid', dxdy=(0, 0), ROI=empty)),
    ])
    device("model.kernel_match", [
        ("search", lambda c: c.model("kernel").match(abc=abc8, quiet=True, search='spiral')), ("grid", lambda c: c.model("kernel").match(abc=abc8, quiet=True, search='grid')),
        ("ROI_and_step", lambda c: c.model("kernel").match(abc=abc8, quiet=True, ROI=((0, 8, 1), (0, 10, 1)), step=2)),
        ("steps_not_positive", lambda c: c.model("kernel").match(abc=abc8, quiet=True, ROI=((0, 8, 1), (0, 10, -1)))),
        ("abc_missing", lambda c: c.model("kernel").match(quiet=True)), ("abc_shape", lambda c: c.model("kernel").match(abc=abc8[:, :9], quiet=True)),
        ("empty", lambda c: c.model("kernel").match(abc=abc8[:0], quiet=True, ROI=((3, 3, 1), (0, 10, 1)))),
        ("beyond_the_extent", lambda c: c.model("kernel").match(abc=np.tile(abc8[:1], (9, 1, 1)), quiet=True, ROI=((0, 9, 1), (0, 10, 1)))),
        ("search+abc", lambda c: c.model("kernel").match(quiet=True, search='spiral')), ("grid+ROI_and_step", lambda c: c.model("kernel").match(quiet=True, search='grid', ROI=whole, step=2)),
        ("steps+abc", lambda c: c.model("kernel").match(quiet=True, ROI=((0, 8, 0), (0, 10, 1)))), ("abc_missing+beyond", lambda c: c.model("kernel").match(quiet=True, ROI=((0, 9, 1), (0, 10, 1)))),
        ("abc_shape+beyond", lambda c: c.model("kernel").match(abc=abc8, quiet=True, ROI=((0, 9, 1), (0, 10, 1)))),
        ("abc_shape+empty", lambda c: c.model("kernel").match(abc=abc8, quiet=True, ROI=((3, 3, 1), (0, 10, 1)))),
        ("uncertainty", lambda c: c.model("kernel").uncertainty(res34)), ("cost_volume", lambda c: c.model("kernel").cost_volume()),
    ])
    device("model.cost_volume", [
        ("masked", lambda c: c.model("masked").cost_volume()), ("pos_list", lambda c: c.model("stepped").cost_volume(with_fit=True)),
        ("masked+ROI", lambda c: c.model("masked").cost_volume(ROI=empty)), ("pos_list+ROI_and_step", lambda c: c.model("stepped").cost_volume(ROI=beyond, step=0)),
    ])
    device("smooth.match_smooth", [
        ("paths", lambda c: smooth.match_smooth(c.model("plain"), paths=6)), ("masked", lambda c: smooth.match_smooth(c.model("masked"))),
        ("max_shift_1", lambda c: smooth.match_smooth(c.model("narrow"))), ("lam_negative", lambda c: smooth.match_smooth(c.model("plain"), lam=-1.0)),
        ("trunc_nan", lambda c: smooth.match_smooth(c.model("plain"), lam=1.0, trunc=NAN)),
        ("paths+masked", lambda c: smooth.match_smooth(c.model("masked"), paths=3)), ("masked+ROI", lambda c: smooth.match_smooth(c.model("masked"), ROI=empty)),
        ("ROI+max_shift", lambda c: smooth.match_smooth(c.model("narrow"), ROI=((3, 3, 1), (0, 16, 1)))), ("max_shift+lam", lambda c: smooth.match_smooth(c.model("narrow"), lam=-1.0)),
    ])
    device("sigma.uncertainty", [
        ("kernel_model", lambda c: sigma.uncertainty(c.model("kernel"), res34)), ("masked", lambda c: sigma.uncertainty(c.model("masked"), res34)),
        ("pos_list", lambda c: sigma.uncertainty(c.model("stepped"), res34)), ("ref_coordinates", lambda c: sigma.uncertainty(c.model("ref_coordinates"), res34)),
        ("noise_var_negative", lambda c: sigma.uncertainty(c.model("plain"), c.result(), noise_var=-1.0)),
        ("maps_of_another_region", lambda c: sigma.uncertainty(c.model("plain"), res34)), ("sam_float32", lambda c: sigma.uncertainty(c.model("plain"), c.result(), sam=sam.astype(np.float32))),
        ("sam_shape", lambda c: sigma.uncertainty(c.model("plain"), c.result(), sam=sam[:, :-1])), ("sam_device_float32", lambda c: sigma.uncertainty(c.model("plain"), c.result(), sam=c.dev(sam.astype(np.float32)))),
        ("sam_device_not_contiguous", lambda c: sigma.uncertainty(c.model("plain"), c.result(), sam=c.strided(sam))), ("staged", lambda c: sigma.uncertainty(c.model("staged"), c.result())),
        ("method", lambda c: c.model("df").uncertainty(res34)),
        ("masked+noise_var", lambda c: sigma.uncertainty(c.model("masked"), res34, noise_var=NAN)), ("noise_var+ROI", lambda c: sigma.uncertainty(c.model("plain"), c.result(), noise_var=INF, ROI=empty)),
        ("ROI+maps", lambda c: sigma.uncertainty(c.model("plain"), res34, ROI=beyond)), ("maps+sam", lambda c: sigma.uncertainty(c.model("plain"), res34, sam=sam[:1])),
        ("maps+staged", lambda c: sigma.uncertainty(c.model("staged"), res34)), ("sam_dtype+shape", lambda c: sigma.uncertainty(c.model("plain"), c.result(), sam=sam[:, :-1].astype(np.float32))),
    ])

    # ------------------------------------------------------------------ ddf.KernelSearch: its region (extent 8 x 10) and its candidates
    cand = [(0.1, 0.0, 0.1)]
    for name, kw in [("steps_not_positive", dict(ROI=((0, 8, 1), (0, 10, -1)))), ("empty", dict(ROI=((3, 3, 1), (0, 10, 1)))), ("beyond_the_extent", dict(ROI=((0, 9, 1), (0, 10, 1)))),
                     ("before_the_extent", dict(ROI=((0, 8, 1), (-2, 10, 1)))), ("step_negative", dict(step=-1)), ("steps+empty", dict(ROI=((3, 3, 0), (0, 10, 1)))),
                     ("empty+beyond", dict(ROI=((0, 9, 1), (5, 5, 1)))), ("ROI_and_step", dict(ROI=((3, 3, 1), (0, 10, 1)), step=2))]:
        row("ddf.KernelSearch.coords:region:" + name, lambda c, kw=kw: c.model("search").coords(**kw), "device")
        row("ddf.KernelSearch.match:region:" + name, lambda c, kw=kw: c.model("search").match(cand, **kw), "device")
    device("ddf.KernelSearch.match", [
        ("no_candidates", lambda c: c.model("search").match([])),
        ("candidates+ROI", lambda c: c.model("search").match([(0.1, 0.0)], ROI=((3, 3, 1), (0, 10, 1)))),
    ])
    return out


def _refused(call):
    try:
        call()
    except RuntimeError:
        return None
    raise AssertionError("the call was not refused")


def observe(row, context=None):
    """Make the call of one row: ``[exception type, complete text]``, or ``["", "returned"]`` where nothing is raised."""
    try:
        row[2](context)
    except Exception as e:                                            # noqa: BLE001 (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return ["", "returned"]
