"""
The calls of the satellite libraries' C ABI that are refused before any device work, one row per ``fail(...)`` of the
sources that an argument alone can reach, and per entry point at least one call that breaks two rules at once (which of
them answers is part of the contract).  tests/golden/make_golden_refusals.py records code and text of every row into
tests/golden/refusals_observed.json; tests/test_refusals_cpu.py replays the rows and compares both exactly.

A row is ``(id, library, function, args, no_device)``.  ``library`` names the accessor of ``umpa_amd._lib``, an argument is
a number, ``None``, a numpy array or a ``ctypes`` array of pointers; ``no_device`` rows pass every argument check and are
answered by the device count, so they hold only where there is no HIP device.

Not reachable without a device, hence not in the table: "device %d out of range" (the count comes first), every text that
carries a HIP error string, register's "no tile ... fits the LDS" (no admitted box reaches it), the null-frame and flag
checks of ``umpa_unwarp_frames`` and the ``uv`` check of ``umpa_grid_match_region`` (they need a map / a model), and a
message longer than the 511 bytes ``fail`` keeps: the longest text an argument can produce is register's flag refusal,
the ``%d`` / ``%g`` / ``%lld`` fields add at most some twenty bytes each, and the only ``%s`` fields are HIP's and
``libumpa_hip.so``'s own error strings.
"""
import ctypes as C

import numpy as np

NAN, INF = float("nan"), float("inf")


def _table(*arrays):
    t = (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data if a is not None else None for a in arrays])
    t.keep = arrays                                      # the table holds addresses only
    return t


def rows():
    out = []

    def row(name, lib, fn, args, no_device=False):
        out.append((name, lib, fn, args, no_device))

    # ------------------------------------------------------------------ umpa_register_sums
    # (a, b, w, dtype, K, H, W, S0, S1, boundary, P, Q, A, device, flags, stream)
    f = np.ones((2, 8, 9))
    s = np.zeros((2, 3, 3))

    def sums(a=f, b=f, w=None, dtype=0, K=2, H=8, W=9, S0=1, S1=1, boundary=0, P=s, Q=s, A=s, device=0, flags=0):
        return [a, b, w, dtype, K, H, W, S0, S1, boundary, P, Q, A, device, flags, None]

    def weights(plane, i, j, value):
        w = np.ones((2, 8, 9))
        w[plane, i, j] = value
        return w

    for name, args in [
        ("null_a", sums(a=None)), ("null_b", sums(b=None)), ("null_P", sums(P=None)), ("null_Q", sums(Q=None)), ("null_A", sums(A=None)),
        ("dtype_3", sums(dtype=3)), ("dtype_negative", sums(dtype=-1)), ("K_negative", sums(K=-1)),
        ("flags_other", sums(flags=2)), ("flags_other_beside_valid", sums(flags=1 | 256 | 512 | 1024)),
        ("boundary_2", sums(boundary=2)), ("boundary_negative", sums(boundary=-1)),
        ("H_zero", sums(H=0)), ("W_zero", sums(W=0)), ("pixels_2_31", sums(H=65536, W=32768)),
        ("S0_negative", sums(S0=-1)), ("S1_negative", sums(S1=-2)),
        ("S0_33", sums(S0=33)), ("S1_40", sums(S1=40)),
        ("box_taller_than_frame", sums(S0=4)), ("box_wider_than_frame", sums(S1=5, S0=0)),
        ("weight_nan", sums(w=weights(1, 2, 3, NAN))), ("weight_negative", sums(w=weights(0, 7, 8, -1.0))),
        ("weight_inf", sums(w=weights(1, 0, 0, INF))),
        # two rules at once
        ("null_a+dtype", sums(a=None, dtype=5)), ("dtype+K", sums(dtype=3, K=-1)), ("K+flags", sums(K=-1, flags=2)),
        ("flags+boundary", sums(flags=2, boundary=2)), ("boundary+H", sums(boundary=2, H=0)), ("H+S0_negative", sums(H=0, S0=-1)),
        ("S0_negative+S1_33", sums(S0=-1, S1=33)), ("S0_33+box", sums(S0=33, H=8)),
        ("box+weight", sums(S0=4, w=weights(0, 0, 0, NAN))), ("weight+device", sums(w=weights(0, 0, 0, NAN), device=-1)),
    ]:
        row("register.sums:" + name, "register", "sums", args)
    row("register.sums:no_device", "register", "sums", sums(), True)
    row("register.sums:no_device+device_negative", "register", "sums", sums(device=-1), True)
    row("register.sums:no_device+K_zero", "register", "sums", sums(K=0), True)
    row("register.sums:no_device+shared_weights_are_one_plane", "register", "sums", sums(w=weights(1, 0, 0, NAN), flags=512), True)

    # ------------------------------------------------------------------ umpa_integrate_vcycle
    # (w, r, z, H, W, device, flags, stream)
    m = np.ones((5, 7))

    def vcycle(w=None, r=m, z=m, H=5, W=7, device=0, flags=0):
        return [w, r, z, H, W, device, flags, None]

    def weight2(i, j, value, shape=(5, 7)):
        w = np.ones(shape)
        w[(Ellipsis, i, j)] = value
        return w

    for name, args in [
        ("null_r", vcycle(r=None)), ("null_z", vcycle(z=None)),
        ("flags_other", vcycle(flags=2)), ("flags_other_beside_valid", vcycle(flags=1 | 256 | 512 | 1024 | 2048)),
        ("H_1", vcycle(H=1)), ("W_1", vcycle(W=1)), ("pixels_2_31", vcycle(H=65536, W=32768)),
        ("weight_nan", vcycle(w=weight2(4, 6, NAN))), ("weight_negative", vcycle(w=weight2(0, 1, -0.5))), ("weight_inf", vcycle(w=weight2(2, 0, INF))),
        ("null_r+flags", vcycle(r=None, flags=2)), ("flags+H", vcycle(flags=2, H=1)), ("H+weight", vcycle(H=1, w=weight2(0, 0, NAN))),
        ("weight+device", vcycle(w=weight2(0, 0, NAN), device=-1)),
    ]:
        row("integrate.vcycle:" + name, "integrate", "vcycle", args)
    row("integrate.vcycle:no_device", "integrate", "vcycle", vcycle(), True)
    row("integrate.vcycle:no_device+device_negative", "integrate", "vcycle", vcycle(device=-1), True)

    # ------------------------------------------------------------------ umpa_integrate_solve
    # (gx, gy, w, K, H, W, tol, maxiter, fill, phi, iters, resid, status, device, flags, stream)
    g = np.ones((2, 5, 7))
    it, st, res = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2)

    def solve(gx=g, gy=g, w=None, K=2, H=5, W=7, tol=1e-10, maxiter=5, phi=g, iters=it, resid=res, status=st, device=0, flags=0):
        return [gx, gy, w, K, H, W, tol, maxiter, 0.0, phi, iters, resid, status, device, flags, None]

    def weight3(k, i, j, value):
        w = np.ones((2, 5, 7))
        w[k, i, j] = value
        return w

    for name, args in [
        ("null_gx", solve(gx=None)), ("null_gy", solve(gy=None)), ("null_phi", solve(phi=None)), ("null_iters", solve(iters=None)),
        ("null_resid", solve(resid=None)), ("null_status", solve(status=None)),
        ("K_negative", solve(K=-3)), ("flags_other", solve(flags=4)), ("H_1", solve(H=1)), ("W_0", solve(W=0)),
        ("pixels_2_31", solve(H=32768, W=65536, K=0)),
        ("tol_nan", solve(tol=NAN)), ("tol_negative", solve(tol=-1e-3)), ("tol_inf", solve(tol=INF)), ("maxiter_negative", solve(maxiter=-1)),
        ("weight_nan", solve(w=weight3(1, 4, 6, NAN))), ("weight_negative", solve(w=weight3(0, 2, 3, -1.0))), ("weight_inf", solve(w=weight3(1, 0, 0, INF))),
        ("null_gx+K", solve(gx=None, K=-1)), ("K+flags", solve(K=-1, flags=4)), ("flags+H", solve(flags=4, H=1)), ("H+tol", solve(H=1, tol=NAN)),
        ("tol+maxiter", solve(tol=-1.0, maxiter=-1)), ("maxiter+weight", solve(maxiter=-1, w=weight3(0, 0, 0, NAN))),
        ("weight+device", solve(w=weight3(0, 0, 0, NAN), device=-1)),
    ]:
        row("integrate.solve:" + name, "integrate", "solve", args)
    row("integrate.solve:no_device", "integrate", "solve", solve(), True)
    row("integrate.solve:no_device+device_negative", "integrate", "solve", solve(device=-1), True)
    row("integrate.solve:no_device+K_zero", "integrate", "solve", solve(K=0), True)

    # ------------------------------------------------------------------ umpa_ddf_kernel (a, b, c, out)
    k = np.zeros(289)
    for name, args in [
        ("null_out", [0.1, 0.0, 0.1, None]), ("a_nan", [NAN, 0.0, 0.1, k]), ("b_inf", [0.1, INF, 0.1, k]), ("c_negative_inf", [0.1, 0.0, -INF, k]),
        ("a_zero", [0.0, 0.0, 0.1, k]), ("c_negative", [0.1, 0.0, -0.25, k]), ("indefinite", [1.0, 3.0, 1.0, k]), ("degenerate", [1.0, 2.0, 1.0, k]),
        ("null_out+a_nan", [NAN, 0.0, 0.1, None]), ("a_nan+c_negative", [NAN, 0.0, -1.0, k]),
    ]:
        row("ddf.kernel:" + name, "ddf", "kernel", args)

    # ------------------------------------------------------------------ umpa_ddf_blur
    # (in, out, K, H, W, kern, device, flags, stream)
    kern = np.full(289, 1.0 / 289)
    fa, fb, oa, ob = np.ones((17, 18)), np.ones((17, 18)), np.zeros((17, 18)), np.zeros((17, 18))
    both = np.ones((2, 17, 18))                          # two adjacent frames of one allocation
    tin, tout = _table(fa, fb), _table(oa, ob)

    def blur(i=tin, o=tout, K=2, H=17, W=18, kn=kern, device=0, flags=0):
        return [i, o, K, H, W, kn, device, flags, None]

    def bad_kernel(q, value):
        b = kern.copy()
        b[q] = value
        return b

    for name, args in [
        ("null_in", blur(i=None)), ("null_out", blur(o=None)), ("null_kernel", blur(kn=None)),
        ("K_negative", blur(K=-1)), ("flags_other", blur(flags=2)), ("H_16", blur(H=16)), ("W_16", blur(W=16)),
        ("rows_beyond_the_grid", blur(K=0, H=65535 * 32 + 1)),
        ("kernel_nan", blur(kn=bad_kernel(5, NAN))), ("kernel_inf", blur(kn=bad_kernel(288, INF))),
        ("frame_null_in", blur(i=_table(fa, None))), ("frame_null_out", blur(o=_table(None, ob))),
        ("alias_same_frame", blur(i=_table(fa, fb), o=_table(oa, fb))), ("alias_across_frames", blur(i=_table(fa, fb), o=_table(fb, oa))),
        ("alias_partial", blur(i=_table(both[0]), o=_table(both.reshape(-1)[17 * 18 - 1:]), K=1)),
        ("null_in+K", blur(i=None, K=-1)), ("K+flags", blur(K=-1, flags=2)), ("flags+H", blur(flags=2, H=16)), ("H+rows", blur(H=65535 * 32 + 1, W=16, K=0)),
        ("rows+kernel", blur(K=0, H=65535 * 32 + 1, kn=bad_kernel(0, NAN))), ("kernel+frame_null", blur(kn=bad_kernel(17, NAN), i=_table(None, fb))),
        ("frame_null+alias", blur(i=_table(fa, None), o=_table(fa, ob))), ("alias+device", blur(o=tin, device=-1)),
    ]:
        row("ddf.blur:" + name, "ddf", "blur", args)
    row("ddf.blur:no_device", "ddf", "blur", blur(), True)
    row("ddf.blur:no_device+device_negative", "ddf", "blur", blur(device=-1), True)
    row("ddf.blur:no_device+K_zero", "ddf", "blur", blur(K=0), True)

    # ------------------------------------------------------------------ umpa_ddf_fold
    # (m, N, f, T, dx, dy, err, best_f, best_T, best_dx, best_dy, index, best_err, device, flags, stream)
    d, e = np.zeros(4), np.zeros(4, dtype=np.int32)

    def fold(m_=0, N=4, missing=None, device=0, flags=0):
        planes = [d, d, d, d, e, d, d, d, d, e, e]
        if missing is not None:
            planes[missing] = None
        return [m_, N] + planes + [device, flags, None]

    for q in range(11):
        row("ddf.fold:null_%d" % q, "ddf", "fold", fold(missing=q))
    for name, args in [
        ("m_negative", fold(m_=-1)), ("N_negative", fold(N=-4)), ("N_2_39", fold(N=1 << 39)), ("flags_other", fold(flags=64)),
        ("null+m", fold(missing=0, m_=-1)), ("m+N", fold(m_=-1, N=-1)), ("N+flags", fold(N=-1, flags=2)), ("flags+device", fold(flags=2, device=-1)),
    ]:
        row("ddf.fold:" + name, "ddf", "fold", args)
    row("ddf.fold:no_device", "ddf", "fold", fold(), True)
    row("ddf.fold:no_device+device_negative", "ddf", "fold", fold(device=-1), True)
    row("ddf.fold:no_device+N_zero", "ddf", "fold", fold(N=0), True)

    # ------------------------------------------------------------------ umpa_unwarp_map_create (H, W, d0, d1, interp, device)
    p = np.zeros((4, 5), dtype=np.float32)

    def plane(i, j, value):
        q = p.copy()
        q[i, j] = value
        return q

    for name, args in [
        ("null_d0", [4, 5, None, p, 0, 0]), ("null_d1", [4, 5, p, None, 0, 0]), ("H_zero", [0, 5, p, p, 0, 0]), ("W_negative", [4, -1, p, p, 0, 0]),
        ("pixels_2_31", [65536, 32768, p, p, 0, 0]), ("interp_2", [4, 5, p, p, 2, 0]), ("interp_negative", [4, 5, p, p, -1, 0]),
        ("d0_nan", [4, 5, plane(3, 4, NAN), p, 0, 0]), ("d1_inf", [4, 5, p, plane(1, 2, INF), 1, 0]),
        ("null+H", [0, 5, None, p, 0, 0]), ("H+interp", [0, 5, p, p, 7, 0]), ("interp+map", [4, 5, plane(0, 0, NAN), p, 2, 0]),
        ("map+device", [4, 5, p, plane(0, 1, NAN), 0, -1]),
    ]:
        row("unwarp.map_create:" + name, "unwarp", "map_create", args)
    row("unwarp.map_create:no_device", "unwarp", "map_create", [4, 5, p, p, 0, 0], True)
    row("unwarp.map_create:no_device+device_negative", "unwarp", "map_create", [4, 5, p, p, 1, -1], True)

    # ------------------------------------------------------------------ umpa_unwarp_frames with a null map, umpa_unwarp_attach with a null model
    # (map, raw, raw_dtype, K, dark, flat, out, flags, stream)
    t = _table(np.zeros((4, 5)))
    for name, args in [
        ("null_map", [None, t, 0, 1, None, None, t, 0, None]), ("null_map+raw", [None, None, 0, 1, None, None, t, 0, None]),
        ("null_map+dtype", [None, t, 3, 1, None, None, t, 0, None]), ("null_map+K+flags", [None, t, 0, -1, None, None, t, 2, None]),
    ]:
        row("unwarp.frames:" + name, "unwarp", "frames", args)
    row("unwarp.attach:null_model", "unwarp", "attach", [None, None])

    # ------------------------------------------------------------------ umpa_grid_* with a null model
    v, ev = np.zeros((7, 4, 4)), np.zeros((4, 4), dtype=np.int32)

    def region(uv=None, flags=0):
        return [None, 0, 1, 4, 0, 1, 4, v, 7, uv, ev, None, 0.0, None, None, None, flags, None]

    row("grid.match_region:null_model", "grid", "match_region", region())
    row("grid.match_region:null_model+uv", "grid", "match_region", region(uv=np.zeros((2, 4, 4))))
    row("grid.match_region:null_model+flags", "grid", "match_region", region(flags=1 << 20))
    c = np.zeros((3, 3, 4, 4))
    row("grid.cost_volume:null_model", "grid", "cost_volume", [None, 0, 1, 4, 0, 1, 4, c, None, None, 0, None])
    row("grid.cost_volume:null_cost", "grid", "cost_volume", [None, 0, 1, 4, 0, 1, 4, None, None, None, 0, None])
    row("grid.cost_volume:null_model+flags", "grid", "cost_volume", [None, 0, 1, 4, 0, 1, 4, c, None, None, 2, None])
    return out


def call(row):
    """Make the call of one row: ``(code, text)``.  ``code`` is the return value; for ``umpa_unwarp_map_create``, which
    returns a handle, it is 0 for NULL and 1 otherwise (a row that is refused gives 0)."""
    from umpa_amd import _lib
    name, libname, fname, args, _ = row
    lib = getattr(_lib, libname)()
    fn = getattr(lib, fname)
    assert len(args) == len(fn.argtypes), name
    conv = []
    for a, typ in zip(args, fn.argtypes):
        if isinstance(a, np.ndarray):
            a = C.cast(C.c_void_p(a.ctypes.data), typ) if typ is not C.c_void_p else C.c_void_p(a.ctypes.data)
        elif isinstance(a, C.Array):
            a = C.cast(a, typ)
        conv.append(a)
    rc = fn(*conv)
    if fn.restype is C.c_void_p:
        if rc:
            lib.map_destroy(rc)
        rc = 1 if rc else 0
    return int(rc), lib.error()
