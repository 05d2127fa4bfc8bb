"""Dumps the three host-side GEMM routing queries of libvitcap_hip.so over a descriptor lattice into tests/golden/gemm_plan.npz:

  vitcap_gemm_plan        -> `rc` [n] and `plan` [n, len(PLAN_FIELDS)] for the descriptors `desc` [n, len(COLS)]
  vitcap_gemm_large_form  -> `large_form` [len(LF_RESERVE), len(LF_HINTS), len(LF_M), len(LF_N), len(LF_K)]
  vitcap_gemm_tile_plan   -> `tile_plan`  [len(LF_M), len(LF_N), len(LF_K), 3]

No GPU is needed (with none the library assumes 256 CUs, an MI355X's count).  The committed file records which kernel every descriptor
launched BEFORE the routing moved into one plan function (docs/LAB_refactor_gemm_plan.md); tests/test_gemm_plan_cpu.py holds the
library to it.  Run from the repository root:  python tests/golden/make_golden_gemm_plan.py [out.npz]
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# one descriptor: vitcap_gemm_desc fields, 0/1 flags for the optional pointers, and the launch-time state the plan reads
COLS = ('M N K lda ldw ldc ldr act out row_group out_group_rows out_row_off res_periodic hint split_k live rowstat colsum ln_bf16 ln_f32 ln_gb '
        'ln_cnt bias res aux ldaux zout ldz reserve defer').split()          # defer: VITCAP_GEMM_4W_DEFER, -1 = unset
PLAN_FIELDS = ('family wm wn stages act out_f32 has_res partial ph mts form mi variant ln_fused ln_follows split_k kt_per_split slab '
               'tiles_m tiles_n n_big tiles_m_small group_n grid_x grid_y grid_z block lds_bytes').split()

HINTS = [0, 1, 2, 4, 5, 13, 14, 15, 20, 21, 22, 23, 24, 30, 31, 32, 33, 40, 41, 42, 3, 12, 43, 99]      # the 20 known ones + 4 unknown
MS = [1, 64, 65, 128, 129, 256, 257, 577, 2047, 2049, 18464, 65536, 295424]
NS = [4, 252, 256, 260, 768, 3072]
KS = [64, 128, 192, 768, 3072]

LF_M = [1000, 2047, 2048, 2049, 4099, 9232, 18464, 36928, 65535, 65536, 73856, 295424]
LF_N = [4, 8, 252, 256, 260, 264, 768, 2304, 3072]
LF_K = [64, 128, 192, 768, 3072]
LF_HINTS = [0, 5, 0x100, 0x105, 1, 42]
LF_RESERVE = [0, 248]


def row(M, N, K, **kw):
    d = dict(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, ldr=N, act=0, out=0, row_group=0, out_group_rows=0, out_row_off=0, res_periodic=0, hint=0,
             split_k=0, live=0, rowstat=0, colsum=0, ln_bf16=0, ln_f32=0, ln_gb=0, ln_cnt=0, bias=1, res=0, aux=0, ldaux=0, zout=0, ldz=0,
             reserve=0, defer=-1)
    for k, v in kw.items():
        assert k in d, k
        d[k] = v
    return [d[c] for c in COLS]


def descriptors():
    rows = []
    # the full hint x M x N x K cross for two epilogues: bf16 plain, fp32 + residual
    for h, M, N, K in itertools.product(HINTS, MS, NS, KS):
        rows.append(row(M, N, K, hint=h))
        rows.append(row(M, N, K, hint=h, out=1, res=1))
    # one factor at a time around a handful of shapes
    base = [(64, 768, 768), (256, 768, 3072), (577, 768, 768), (2049, 256, 192), (2049, 260, 192), (18464, 2304, 768), (65536, 3072, 768)]
    hints = [0, 5, 4, 13, 20, 23, 33, 40, 41, 42]
    for (M, N, K), h in itertools.product(base, hints):
        rows.append(row(M, N, K, hint=h, out=1, rowstat=1))
        for out, res in ((0, 0), (1, 1)):
            e = dict(hint=h, out=out, res=res)
            for act in (1, 2):
                rows.append(row(M, N, K, act=act, **e))
            for sk in (2, 6):
                rows.append(row(M, N, K, split_k=sk, bias=0, **e))
            rows.append(row(M, N, K, rowstat=1, **e))
            rows.append(row(M, N, K, colsum=1, **e))
            rows.append(row(M, N, K, aux=1, ldaux=N, **e))
            rows.append(row(M, N, K, aux=1, ldaux=N + 4, **e))
            rows.append(row(M, N, K, zout=1, ldz=N, act=1, **e))
            rows.append(row(M, N, K, zout=1, ldz=N + 4, act=1, **e))
            rows.append(row(M, N, K, ln_bf16=1, ln_gb=1, **e))
            rows.append(row(M, N, K, ln_bf16=1, ln_f32=1, ln_gb=1, ln_cnt=1, **e))
            rows.append(row(M, N, K, row_group=576, out_group_rows=577, out_row_off=1, res_periodic=1, **e))
            rows.append(row(M, N, K, live=1, **e))
            rows.append(row(M, N, K, ldc=N + 4, ldr=N + 4, **e))
            for rsv, df in itertools.product((0, 248), (-1, 0, 1, 2)):
                if rsv or df >= 0:
                    rows.append(row(M, N, K, reserve=rsv, defer=df, **e))
    # the LayerNorm behind (or inside) the GEMM: N = 768 is the only width it admits
    for M, K, h, res, cnt in itertools.product((64, 577, 2047, 2048, 18464), (768, 3072), hints, (0, 1), (0, 1)):
        rows.append(row(M, 768, K, hint=h, out=1, res=res, ln_bf16=1, ln_gb=1, ln_cnt=cnt))
    return np.asarray(rows, dtype=np.int64)


class _State:
    """reserve / VITCAP_GEMM_4W_DEFER as a descriptor row asks for them; restored on exit"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.env = os.environ.get('VITCAP_GEMM_4W_DEFER')
        self.prev = self.lib.vitcap_gemm_reserve_cus(0)
        return self

    def set(self, reserve, defer):
        self.lib.vitcap_gemm_reserve_cus(int(reserve))
        # os.environ writes through to the C environment the library's getenv reads
        if defer < 0:
            os.environ.pop('VITCAP_GEMM_4W_DEFER', None)
        else:
            os.environ['VITCAP_GEMM_4W_DEFER'] = str(int(defer))

    def __exit__(self, *exc):
        self.lib.vitcap_gemm_reserve_cus(self.prev)
        if self.env is None:
            os.environ.pop('VITCAP_GEMM_4W_DEFER', None)
        else:
            os.environ['VITCAP_GEMM_4W_DEFER'] = self.env


def query_plans(L, desc):
    """vitcap_gemm_plan for every row of `desc` (columns COLS): (rc [n], plan [n, len(PLAN_FIELDS)], zeros where rc != 0).  The optional
    pointers are small fake addresses: the query reads none of them."""
    fake = lambda on, k: C.c_void_p(0x1000 * (k + 1)) if on else None
    rc = np.zeros(len(desc), dtype=np.int32)
    plan = np.zeros((len(desc), len(PLAN_FIELDS)), dtype=np.int64)
    info = L.GemmPlanInfo()
    with _State(L.lib) as st:
        for i, r in enumerate(desc.tolist()):
            v = dict(zip(COLS, r))
            d = L.GemmDesc(M=v['M'], N=v['N'], K=v['K'], lda=v['lda'], ldw=v['ldw'], ldc=v['ldc'], ldr=v['ldr'], act=v['act'], out_dtype=v['out'],
                           row_group=v['row_group'], out_group_rows=v['out_group_rows'], out_row_off=v['out_row_off'], res_periodic=v['res_periodic'],
                           tile_hint=v['hint'], split_k=v['split_k'], live=fake(v['live'], 0), rowstat=fake(v['rowstat'], 1), colsum=fake(v['colsum'], 2),
                           ln_gamma=fake(v['ln_gb'], 3), ln_beta=fake(v['ln_gb'], 4), ln_eps=1e-6, ln_out_bf16=fake(v['ln_bf16'], 5),
                           ln_out_f32=fake(v['ln_f32'], 6), ln_counters=fake(v['ln_cnt'], 7))
            st.set(v['reserve'], v['defer'])
            rc[i] = L.lib.vitcap_gemm_plan(C.byref(d), v['bias'], v['res'], v['aux'], v['ldaux'], v['zout'], v['ldz'], C.byref(info))
            if rc[i] == 0:
                grid = dict(grid_x=info.grid[0], grid_y=info.grid[1], grid_z=info.grid[2])
                plan[i] = [grid[f] if f in grid else getattr(info, f) for f in PLAN_FIELDS]
    return rc, plan


def query_large(L):
    lf = np.zeros((len(LF_RESERVE), len(LF_HINTS), len(LF_M), len(LF_N), len(LF_K)), dtype=np.int32)
    tp = np.zeros((len(LF_M), len(LF_N), len(LF_K), 3), dtype=np.int32)
    p3 = (C.c_int * 3)()
    with _State(L.lib) as st:
        for (ir, rsv), (ih, h), (im, M), (i_n, N), (ik, K) in itertools.product(*(list(enumerate(a)) for a in (LF_RESERVE, LF_HINTS, LF_M, LF_N, LF_K))):
            st.set(rsv, -1)
            lf[ir, ih, im, i_n, ik] = L.lib.vitcap_gemm_large_form(M, N, K, h)
        for (im, M), (i_n, N), (ik, K) in itertools.product(*(list(enumerate(a)) for a in (LF_M, LF_N, LF_K))):
            assert L.lib.vitcap_gemm_tile_plan(M, N, K, p3) == 0
            tp[im, i_n, ik] = list(p3)
    return lf, tp


def dump(L):
    desc = descriptors()
    rc, plan = query_plans(L, desc)
    lf, tp = query_large(L)
    return dict(desc=desc.astype(np.int32), rc=rc, plan=plan.astype(np.int32), large_form=lf, tile_plan=tp)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from vitcap_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'gemm_plan.npz')
    arrays = dump(_lib)
    np.savez_compressed(out, **arrays)
    print(out, {k: v.shape for k, v in arrays.items()}, os.path.getsize(out), 'bytes')
