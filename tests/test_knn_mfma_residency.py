"""knn_mfma.hip's residency budget at the bench shape (B 32, N 1024, k 20), read from the code objects (tools/kernel_meta.py):
the whole grid must be resident in ONE round on 256 CUs with a Chamfer search workgroup beside it on every CU.  A kernel that
needs a second round (the 69.6 KB / 199-VGPR kernel of round 6 ran two) is 8-10 us slower and keeps the Chamfer branch from
overlapping it.  Also a model of the pop's register -> staged-slot mapping against the staging scatter.  No GPU needed."""
import ctypes
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CUS = 256                       # MI355X
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512            # per lane, wave64 (VGPRs + AGPRs)
QUERIES_PER_WG, WAVES_PER_WG = 64, 8


def _meta():
    from learning3d_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    return km.kernel_metadata(_lib.LIB_PATH)


def _one(meta, prefix):
    ks = [k for n, k in meta.items() if n.startswith(prefix)]
    assert len(ks) == 1, prefix
    return ks[0]


def _lds_bytes(N):
    from learning3d_amd import _lib
    f = getattr(_lib.lib(), "_Z22l3d_knn_mfma_lds_bytesi")
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int]
    return int(f(N))


def _regs(k):
    return -(-(k[".vgpr_count"] + k.get(".agpr_count", 0)) // 8) * 8        # allocation granule: 8 registers


def test_knn_mfma_bench_shape_is_one_round_beside_chamfer():
    meta = _meta()
    knn = _one(meta, "_Z15knn_mfma_kernelILi8EE")                          # 896 < N <= 1024
    assert knn[".max_flat_workgroup_size"] == 64 * WAVES_PER_WG
    assert knn[".vgpr_count"] + knn.get(".agpr_count", 0) <= 128            # 4 waves per SIMD
    lds = _lds_bytes(1024)
    assert lds <= 60 * 1024, lds                                           # 59 664 B today
    wgs = (1024 // QUERIES_PER_WG) * 32                                     # B 32
    per_cu = -(-wgs // CUS)
    assert per_cu == 2
    waves_per_simd = per_cu * WAVES_PER_WG // 4
    chamfer = [k for n, k in meta.items() if n.startswith("_Z25chamfer_fwd_packed_kernel")]
    assert len(chamfer) >= 2
    for ch in chamfer:                                                      # either tile size: one search workgroup fits beside
        assert per_cu * lds + ch[".group_segment_fixed_size"] <= LDS_PER_CU, (lds, ch[".name"])
        assert waves_per_simd * _regs(knn) + _regs(ch) <= VGPRS_PER_SIMD, (_regs(knn), ch[".name"])


def test_knn_mfma_lds_fits_two_workgroups_at_every_supported_n():
    for N in (256, 257, 1000, 1024, 1025, 1500, 2048):
        assert 2 * _lds_bytes(N) <= LDS_PER_CU, N


def test_knn_mfma_pop_slot_model():
    """Pass 1 rebuilds a hit's value from the staged cloud: register e & 15 of tile j + (e >> 4) of lane (i, h) in wave wq
    of a half is staged slot wq WS + 4 h + 32 j + e + (e & ~3), and that slot must hold candidate 128 j + 8 e + lane8
    (what the key's index says) -- the staging scatter's own formula, checked for every (wave, h, tile pair, e)."""
    for T in (2, 3, 8, 16):
        WS = T * 32 + 16
        slot_of = {}
        for c in range(4 * T * 32):
            l8, s = c & 7, c >> 3
            jj, r = s >> 4, s & 15
            slot_of[(l8 >> 1) * WS + jj * 32 + ((r >> 2) << 3) + ((l8 & 1) << 2) + (r & 3)] = c
        for wq in range(4):
            for h in range(2):
                lane8 = 2 * wq + h
                for j in range(0, T, 2):
                    for e in range(32 if j + 1 < T else 16):
                        p = wq * WS + 4 * h + 32 * j + e + (e & ~3)
                        assert slot_of[p] == 128 * j + 8 * e + lane8, (T, wq, h, j, e)
                        tile, r = j + (e >> 4), e & 15                  # the 32x32x2 accumulator layout: row 8 (r / 4) + 4 h + r % 4
                        assert p == wq * WS + tile * 32 + 8 * (r >> 2) + 4 * h + (r & 3)
