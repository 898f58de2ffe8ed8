"""ctypes loader of tests/probe/libpp_expand_probe.so: the small algorithms of path_planner_amd/csrc/pp_k_expand.h, each alone, with
numpy in and numpy out.  __graft_entry__.build() compiles the library; PP_EXPAND_PROBE_LIB points at another build of it (a copy of
csrc/ with one piece changed on purpose, to see that the tests notice)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "probe", "libpp_expand_probe.so")
WAVE = 64

_lib = []


def lib_path():
    return os.environ.get("PP_EXPAND_PROBE_LIB") or DEFAULT_LIB


def lib():
    if not _lib:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run build() (python __graft_entry__.py) first")
        L = C.CDLL(path)
        vp, ll, i32, dbl = C.c_void_p, C.c_longlong, C.c_int, C.c_double
        for name, args in [
            ("ppe_heap_replay", [vp, vp, vp, i32, vp, vp]), ("ppe_kth_wave", [vp, vp, vp, i32, vp]),
            ("ppe_kth_lds", [vp, vp, vp, vp, i32, dbl, i32, vp, vp]), ("ppe_rank_lds", [vp, vp, i32, vp, vp, i32, vp]),
            ("ppe_k_smallest", [i32, vp, vp, vp, vp, vp, i32, vp, vp]),
            ("ppe_wg_append_one_list8", [vp, i32, vp, vp, i32, vp]), ("ppe_wg_append_two_lists", [vp, i32, vp, vp, i32, vp]),
            ("ppe_expand_bound", [vp, vp, i32, i32, vp, vp]),
            ("ppe_half_wave_min", [vp, vp, ll]), ("ppe_ord_sort", [vp, vp, vp, i32, i32, i32, vp, vp]),
        ]:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _cat(arrays, dtype):
    return np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays] + [np.zeros(0, dtype=dtype)]))


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def heap_replay(cost_lists, ks):
    """Per case (a cost sequence, k): pp_ord_sift_up of entry i, pp_ord_pop once the heap holds k + 1.  Returns per case the heap
    array after every operation (nops x k, -1 beyond its size) and pp_ord_safe's verdict after every operation (1 / 0; -1 while the
    heap is not full)."""
    ks = _i32(ks)
    nops = _i32([len(c) for c in cost_lists])
    costs = _cat(cost_lists, np.float64)
    idx = np.full(int((nops.astype(np.int64) * ks).sum()), -7, dtype=np.int32)
    safe = np.full(int(nops.sum()), -7, dtype=np.int32)
    _ck(lib().ppe_heap_replay(_p(costs), _p(nops), _p(ks), len(ks), _p(idx), _p(safe)), "ppe_heap_replay")
    out, a, b = [], 0, 0
    for n, k in zip(nops.tolist(), ks.tolist()):
        out.append((idx[a:a + n * k].reshape(n, k), safe[b:b + n]))
        a += n * k
        b += n
    return out


def kth_wave(x, n, k):
    """x: cases x 64 (one value per lane), n / k per case -> cases x 64: what every lane got from pp_kth_smallest_wave."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, WAVE)
    n, k = _i32(n), _i32(k)
    out = np.full_like(x, np.nan)
    _ck(lib().ppe_kth_wave(_p(x), _p(n), _p(k), x.shape[0], _p(out)), "ppe_kth_wave")
    return out


def kth_lds(L_lists, I_lists, ks, sentinel_l, sentinel_i):
    """pp_kth_smallest_lds per case; I_lists None: the form without an index array (ties by position).  -> (kthL, kthI) per case."""
    n = _i32([len(l) for l in L_lists])
    L = _cat(L_lists, np.float64)
    I = None if I_lists is None else _cat(I_lists, np.int32)
    ks = _i32(ks)
    outL, outI = np.zeros(len(ks)), np.zeros(len(ks), dtype=np.int32)
    _ck(lib().ppe_kth_lds(_p(L), _p(I) if I is not None else None, _p(n), _p(ks), len(ks), float(sentinel_l), int(sentinel_i), _p(outL), _p(outI)),
        "ppe_kth_lds")
    return outL, outI


def rank_lds(L, I, x, xi):
    """pp_rank_lds of every query (x, xi) against one list; I None: ties by position."""
    L, x, xi = _f64(L), _f64(x), _i32(xi)
    I = None if I is None else _i32(I)
    out = np.full(x.size, -7, dtype=np.int32)
    _ck(lib().ppe_rank_lds(_p(L), _p(I) if I is not None else None, L.size, _p(x), _p(xi), x.size, _p(out)), "ppe_rank_lds")
    return out


def k_smallest(nt, L_lists, I_lists, valid_lists, ks, with_lengths=True, prefill=-99):
    """pp_k_smallest<nt> per case over entries (L, I, valid).  -> per case (indices[k], lengths[k] or None); slots the kernel did not
    write keep `prefill`."""
    n = _i32([len(l) for l in L_lists])
    L, I, V = _cat(L_lists, np.float64), _cat(I_lists, np.int32), _cat(valid_lists, np.uint8)
    ks = _i32(ks)
    oi = np.full(int(ks.sum()), prefill, dtype=np.int32)
    ol = np.full(int(ks.sum()), float(prefill)) if with_lengths else None
    _ck(lib().ppe_k_smallest(nt, _p(L), _p(I), _p(V), _p(n), _p(ks), len(ks), _p(oi), _p(ol) if with_lengths else None), "ppe_k_smallest")
    out, a = [], 0
    for k in ks.tolist():
        out.append((oi[a:a + k], ol[a:a + k] if with_lengths else None))
        a += k
    return out


def wg_append(one_list, take, count0, cap):
    """take: workgroups x R x 256 flags (R = 8 with one_list, else 2).  -> (counters after, lists [lists][cap] with -1 where nothing
    was written, flags whose slot fell outside the list).  An id in a list = (workgroup * R + flag) * 256 + thread."""
    R, lists = (8, 1) if one_list else (2, 2)
    take = np.ascontiguousarray(take, dtype=np.uint8)
    assert take.ndim == 3 and take.shape[1:] == (R, 256)
    count = _i32(count0).copy()
    assert count.size == lists
    out = np.full((lists, cap), -1, dtype=np.int32)
    bad = np.zeros(1, dtype=np.int32)
    fn = lib().ppe_wg_append_one_list8 if one_list else lib().ppe_wg_append_two_lists
    _ck(fn(_p(take), take.shape[0], _p(count), _p(out), cap, _p(bad)), "ppe_wg_append")
    return count, out, int(bad[0])


def half_wave_min(x):
    x = _f64(x)
    n = x.size
    padded = np.full((n + 255) // 256 * 256, np.inf)
    padded[:n] = x
    out = np.full_like(padded, np.nan)
    _ck(lib().ppe_half_wave_min(_p(padded), _p(out), padded.size), "ppe_half_wave_min")
    return out[:n], padded


def expand_bound(groupmin, groupcnt, near_count, k):
    """The kernel pp_k_expand_bound on one vertex's group minima (groups x 2, +inf = no valid slot) and slots in use per group.
    -> (U per radius, the two candidate counters, handed in as 7 and 9)."""
    gm = np.ascontiguousarray(groupmin, dtype=np.float64).reshape(-1, 2)
    gc = _i32(groupcnt)
    assert gm.shape[0] == gc.size == (near_count + 31) // 32
    bound, count = np.array([-5.0, -5.0]), np.array([7, 9], dtype=np.int32)
    _ck(lib().ppe_expand_bound(_p(gm), _p(gc), int(near_count), int(k), _p(bound), _p(count)), "ppe_expand_bound")
    return bound, count


def ord_sort(cd, ci, val):
    """pp_ord_sort of Mk kept candidates (distance cd, list position ci) of a list whose samples are val.  -> (cd, ci) of the n2
    slots the sort works on, the padding included."""
    cd, ci, val = _f64(cd), _i32(ci), _i32(val)
    n2 = 64
    while n2 < cd.size:
        n2 <<= 1
    ocd, oci = np.full(n2, np.nan), np.full(n2, -7, dtype=np.int32)
    _ck(lib().ppe_ord_sort(_p(cd), _p(ci), _p(val), cd.size, val.size, n2, _p(ocd), _p(oci)), "ppe_ord_sort")
    return ocd, oci
