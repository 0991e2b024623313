"""The grid of tests/golden/launch_plan_table.npz and the replay of the public planning calls over it.

The table is a recording of the planning calls' answers at the commit before the launch plan was introduced
(sw_plan_query, sw_plan_launch, sw_launch_vgpr_slot, sw_scan_temp_bytes, sw_rescore_service_temp_bytes,
sw_packed_launch_falls_back), made on an MI355X, one process per context variant.  Arrays of a variant are indexed
[query type][query length][kind][part_id][n][max_subject_len]; the service sizes [query type][query length][kind]
[max_subject_len][workgroups]; sw_plan_query's answers [kind][query length]."""
import ctypes
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan_table.npz")

KINDS = (0, 1, 2, 3)
QLENS = (1, 64, 96, 97, 128, 129, 256, 257, 512, 576, 577, 768, 769, 1000, 1536, 1537, 2048, 5478, 35213)
PARTS = (-1, 0, 10, 33, 34, 35)
NS = (1, 100, 511, 512, 5000, 125000, 1000000)
MSLS = (64, 192, 193, 320, 321, 1024, 1025, 1280, 1281, 8000, 35000, 65535, 70000)
GAPS = ((-11, -1), (-10, -2), (-5, -13), (0, 0))
SERVICE_WGS = (1, 8, 64)
QTYPES = ("letters", "pssm")
MATRIX_MAX = 11   # the letter queries' matrix: 11 on the diagonal, -1 elsewhere
PSSM_MAX = 20     # the PSSM queries: one entry of 20 per row, -1 elsewhere

VARIANTS = (
    ("default", {}),
    ("chain1", {"CUDASW4_AMD_CHAIN": "1"}),
    ("chain4_all", {"CUDASW4_AMD_CHAIN": "4", "CUDASW4_AMD_CHAIN_ALL": "1"}),
    ("stream1", {"CUDASW4_AMD_STREAM": "1"}),
    ("no_offs", {"CUDASW4_AMD_NO_OFFS": "1"}),
    ("i32_native", {"CUDASW4_AMD_I32_NATIVE": "1"}),
    ("lanes8_0_lanes4_64", {"CUDASW4_AMD_LANES8_MAX_Q": "0", "CUDASW4_AMD_LANES4_MAX_Q": "64"}),
    ("grid_cap8", {"CUDASW4_AMD_GRID_CAP": "8"}),
)
LAUNCH_FIELDS = ("rc", "eff_kind", "rows", "nstripes", "lanes", "slot", "temp", "falls_back")


def matrix21():
    m = np.full((21, 21), -1, dtype=np.int8)
    np.fill_diagonal(m, MATRIX_MAX)
    m[20, :] = -1
    m[:, 20] = -1
    return m


def letters(qlen):
    return (np.arange(qlen, dtype=np.int64) * 7 % 20).astype(np.int8)


def pssm(qlen):
    p = np.full((qlen, 21), -1, dtype=np.int8)
    p[np.arange(qlen), np.arange(qlen) % 20] = PSSM_MAX
    return p


def empty_tables():
    shape = (len(QTYPES), len(QLENS), len(KINDS), len(PARTS), len(NS), len(MSLS))
    t = {
        "rc": np.zeros(shape, np.int8), "eff_kind": np.full(shape, -1, np.int8), "rows": np.zeros(shape, np.int16),
        "nstripes": np.zeros(shape, np.int32), "lanes": np.zeros(shape, np.int8), "slot": np.zeros(shape, np.int16),
        "temp": np.zeros(shape, np.int64), "falls_back": np.zeros(shape, np.int8),
        "service": np.zeros((len(QTYPES), len(QLENS), len(KINDS), len(MSLS), len(SERVICE_WGS)), np.int64),
    }
    return t


def plan_query_table(lib):
    """sw_plan_query over [kind][query length]: (rc, rows, nstripes)"""
    i32 = ctypes.c_int32
    lib.sw_plan_query.argtypes = [ctypes.c_int, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    out = np.zeros((len(KINDS), len(QLENS), 3), np.int32)
    r, s = i32(0), i32(0)
    for ki, kind in enumerate(KINDS):
        for qi, qlen in enumerate(QLENS):
            rc = lib.sw_plan_query(kind, qlen, ctypes.byref(r), ctypes.byref(s))
            out[ki, qi] = (rc, r.value, s.value)
    return out


def record(lib, device=0):
    """One context (created now: the environment's tuning variables are read here), every call over the grid."""
    vp, i32, ci, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int, ctypes.c_size_t
    p32 = ctypes.POINTER(i32)
    lib.sw_ctx_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.sw_ctx_destroy.argtypes = [vp]
    lib.sw_set_matrix.argtypes = [vp, vp, ci]
    lib.sw_set_query.argtypes = [vp, vp, i32, vp]
    lib.sw_set_query_pssm.argtypes = [vp, vp, i32, vp]
    lib.sw_plan_launch.argtypes = [vp, ci, ci, i32, i32, p32, p32, p32, p32]
    lib.sw_launch_vgpr_slot.argtypes = [vp, ci, ci, i32, i32]
    lib.sw_scan_temp_bytes.argtypes = [vp, ci, ci, i32, i32]
    lib.sw_scan_temp_bytes.restype = sz
    lib.sw_rescore_service_temp_bytes.argtypes = [vp, ci, i32, ci]
    lib.sw_rescore_service_temp_bytes.restype = sz
    lib.sw_packed_launch_falls_back.argtypes = [vp, ci, ci, i32, i32, ci, ci]
    lib.sw_last_error.restype = ctypes.c_char_p
    ctx = vp()
    rc = lib.sw_ctx_create(device, ctypes.byref(ctx))
    assert rc == 0, lib.sw_last_error()
    t = empty_tables()
    try:
        m = matrix21()
        assert lib.sw_set_matrix(ctx, m.ctypes.data, 21) == 0, lib.sw_last_error()
        ek, ro, ns, la = i32(0), i32(0), i32(0), i32(0)
        bek, bro, bns, bla = (ctypes.byref(x) for x in (ek, ro, ns, la))
        plan, slot, temp, fb, service = (lib.sw_plan_launch, lib.sw_launch_vgpr_slot, lib.sw_scan_temp_bytes,
                                         lib.sw_packed_launch_falls_back, lib.sw_rescore_service_temp_bytes)
        for ti in range(len(QTYPES)):
            for qi, qlen in enumerate(QLENS):
                if ti == 0:
                    q = letters(qlen)
                    assert lib.sw_set_query(ctx, q.ctypes.data, qlen, None) == 0, lib.sw_last_error()
                else:
                    q = pssm(qlen)
                    assert lib.sw_set_query_pssm(ctx, q.ctypes.data, qlen, None) == 0, lib.sw_last_error()
                for ki, kind in enumerate(KINDS):
                    for mi, msl in enumerate(MSLS):
                        for wi, wg in enumerate(SERVICE_WGS):
                            t["service"][ti, qi, ki, mi, wi] = service(ctx, kind, msl, wg)
                    for pi, part in enumerate(PARTS):
                        for ni, n in enumerate(NS):
                            for mi, msl in enumerate(MSLS):
                                ix = (ti, qi, ki, pi, ni, mi)
                                ek.value = -1; ro.value = 0; ns.value = 0; la.value = 0
                                t["rc"][ix] = plan(ctx, kind, part, n, msl, bek, bro, bns, bla)
                                t["eff_kind"][ix] = ek.value
                                t["rows"][ix] = ro.value
                                t["nstripes"][ix] = ns.value
                                t["lanes"][ix] = la.value
                                t["slot"][ix] = slot(ctx, kind, part, n, msl)
                                t["temp"][ix] = temp(ctx, kind, part, n, msl)
                                bits = 0
                                for gi, (gop, gex) in enumerate(GAPS):
                                    bits |= (1 if fb(ctx, kind, part, n, msl, gop, gex) else 0) << gi
                                t["falls_back"][ix] = bits
    finally:
        lib.sw_ctx_destroy(ctx)
    return t
