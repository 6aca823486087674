"""Packed projection / sparse gradients, the part that needs no GPU: the reference helper itself, the C ABI's argument
validation and marshalling, how the operators fail on CPU tensors, and the new kernels' resource remarks."""
import os

import pytest
import torch

from oracle import gsplat_oracle as G
from tests import packed_ref
from tests.scenes import random_scene, small_pose
from tests.test_kernel_resources import HIPCC, _resources

BAD_ARG, WORKSPACE, HIP = -1, -2, -3


def test_pack_of_the_oracle_equals_a_loop_over_pairs():
    """pack() of the float64 oracle's dense projection on a 3-camera scene against a hand-written loop over
    (camera, Gaussian) pairs: pins the helper every GPU test of packed mode relies on."""
    N, W, H = 300, 64, 48
    sc = random_scene(N, W, H, seed=5, sigma_px=1.5, aniso=True)
    sc["means"][:, :2] *= 2.0  # part of the cloud outside every frustum
    Vs = torch.stack([torch.linalg.inv(small_pose(4.0, 0.3, seed=s)) for s in (1, 2, 3)])
    Ks = sc["K"][None].expand(3, 3, 3)
    dense = G.fully_fused_projection(sc["means"], sc["quats"], sc["scales"], Vs, Ks, W, H, calc_compensations=True)
    got = packed_ref.pack(dense)
    rows = {k: [] for k in packed_ref.NAMES}
    for c in range(3):
        for i in range(N):
            if int(dense[0][c, i]) > 0:
                rows["camera_ids"].append(c)
                rows["gaussian_ids"].append(i)
                for k, t in zip(packed_ref.NAMES[2:], dense):
                    rows[k].append(t[c, i])
    nnz = len(rows["camera_ids"])
    assert 0 < nnz < 3 * N  # some pairs culled, some kept
    assert got["camera_ids"].dtype == torch.int64 and got["gaussian_ids"].dtype == torch.int64
    assert got["camera_ids"].tolist() == rows["camera_ids"] and got["gaussian_ids"].tolist() == rows["gaussian_ids"]
    for k in packed_ref.NAMES[2:]:
        assert torch.equal(got[k], torch.stack(rows[k])), k
    flat = got["camera_ids"] * N + got["gaussian_ids"]
    assert bool((flat[1:] > flat[:-1]).all())
    assert packed_ref.pack(dense[:4] + (None,))["compensations"] is None


def _lib():
    from gsplatloc_amd import _lib as L

    return L.load_library()


def test_packed_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib()
    f32 = lambda *s: torch.zeros(*s)  # noqa: E731
    from gsplatloc_amd._lib import ptr

    N, C = 100, 2
    m, q, s, V, K = f32(N, 3), f32(N, 4), f32(N, 3), f32(C, 4, 4), f32(C, 3, 3)
    ws_bytes = lib.gsl_project_packed_ws_bytes(C, N)
    assert ws_bytes == 1 * (4 * 8 + 2 * 4) and lib.gsl_project_packed_ws_bytes(4, 1000) == 16 * 40
    assert lib.gsl_project_packed_ws_bytes(0, 0) == 40
    ws, nnz = torch.zeros(ws_bytes, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    head = (ptr(m), ptr(q), ptr(s), ptr(V), ptr(K))
    tail = (64, 48, 0.3, 0.01, 1e10, 0.0)
    count = lib.gsl_project_packed_count
    assert count(*head, C, N, *tail, None, ptr(ws), ws_bytes, None) == BAD_ARG             # no nnz
    assert count(*head, 0, N, *tail, ptr(nnz), ptr(ws), ws_bytes, None) == BAD_ARG         # no camera
    assert count(*head, C, -1, *tail, ptr(nnz), ptr(ws), ws_bytes, None) == BAD_ARG
    assert count(*head, C, N, 0, 48, 0.3, 0.01, 1e10, 0.0, ptr(nnz), ptr(ws), ws_bytes, None) == BAD_ARG
    assert count(None, *head[1:], C, N, *tail, ptr(nnz), ptr(ws), ws_bytes, None) == BAD_ARG
    assert count(*head, 1 << 12, 1 << 20, *tail, ptr(nnz), ptr(ws), 1 << 40, None) == BAD_ARG  # C * N >= 2^31
    assert count(*head, C, N, *tail, ptr(nnz), ptr(ws), ws_bytes - 1, None) == WORKSPACE
    assert count(*head, C, N, *tail, ptr(nnz), None, ws_bytes, None) == WORKSPACE
    fill = lib.gsl_project_packed_fill
    ids, rad = torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)
    outs = (ptr(ids), ptr(ids), ptr(rad), ptr(f32(8, 2)), ptr(f32(8)), ptr(f32(8, 3)), None)
    assert fill(*head, C, N, *tail, -1, *outs, ptr(ws), ws_bytes, None) == BAD_ARG
    assert fill(*head, C, N, *tail, 8, None, *outs[1:], ptr(ws), ws_bytes, None) == BAD_ARG
    assert fill(*head, C, N, *tail, 8, *outs, ptr(ws), ws_bytes - 8, None) == WORKSPACE
    assert fill(*head, C, N, *tail, 0, *outs, ptr(ws), ws_bytes, None) == 0                 # nothing kept: no launch
    bwd = lib.gsl_project_packed_bwd
    assert lib.gsl_project_packed_bwd_ws_bytes(1000, 3) == (4 + 3 - 1) * 12 * 4
    assert lib.gsl_project_packed_bwd_ws_bytes(0, 1) == 12 * 4
    bws_bytes = lib.gsl_project_packed_bwd_ws_bytes(8, C)
    bws = torch.zeros(bws_bytes, dtype=torch.uint8)
    rows = (ptr(ids), ptr(ids), ptr(f32(8, 3)), None, ptr(f32(8, 2)), ptr(f32(8)), ptr(f32(8, 3)), None)
    grads = (ptr(f32(N, 3)), ptr(f32(N, 4)), ptr(f32(N, 3)), ptr(f32(C, 4, 4)))
    assert bwd(*head, C, N, 64, 48, 0.3, -1, *rows, 0, *grads, ptr(bws), bws_bytes, None) == BAD_ARG
    assert bwd(*head, C, N, 64, 48, 0.3, C * N + 1, *rows, 0, *grads, ptr(bws), 1 << 30, None) == BAD_ARG
    assert bwd(*head, C, N, 64, 48, 0.3, 8, *rows, 0, grads[0], None, *grads[2:], ptr(bws), bws_bytes, None) == BAD_ARG
    assert bwd(*head, C, N, 64, 48, 0.3, 8, *rows[:7], ptr(f32(8)), 0, *grads, ptr(bws), bws_bytes, None) == BAD_ARG
    assert bwd(*head, C, N, 64, 48, 0.3, 8, None, *rows[1:], 0, *grads, ptr(bws), bws_bytes, None) == BAD_ARG
    assert bwd(*head, C, N, 64, 48, 0.3, 8, *rows, 0, *grads, ptr(bws), bws_bytes - 4, None) == WORKSPACE
    # the row gather and its vjp
    src, dst = f32(N, 3), f32(8, 3)
    assert lib.gsl_gather_rows(ptr(src), N, 0, ptr(ids), 8, ptr(dst), None) == BAD_ARG          # no floats per row
    assert lib.gsl_gather_rows(ptr(src), N, 3, None, 8, ptr(dst), None) == BAD_ARG
    assert lib.gsl_gather_rows(ptr(src), N, 3, ptr(ids), -1, ptr(dst), None) == BAD_ARG
    assert lib.gsl_gather_rows(ptr(src), N, 3, ptr(ids), 1 << 31, ptr(dst), None) == BAD_ARG
    assert lib.gsl_gather_rows(ptr(src), N, 3, ptr(ids), 0, None, None) == 0                    # nothing to do
    assert lib.gsl_scatter_add_rows(ptr(dst), ptr(ids), 8, 3, N, 0, None, None) == BAD_ARG
    assert lib.gsl_scatter_add_rows(None, ptr(ids), 8, 3, N, 0, ptr(src), None) == BAD_ARG
    assert lib.gsl_scatter_add_rows(ptr(dst), ptr(ids), 8, 3, 1 << 31, 0, ptr(src), None) == BAD_ARG
    assert lib.gsl_scatter_add_rows(ptr(dst), ptr(ids), 8, 0, N, 1, ptr(src), None) == BAD_ARG


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-pointer calls: only meaningful without a GPU")
def test_packed_entry_points_marshal():
    """Valid argument lists on host tensors: ctypes accepts them, validation passes, the HIP runtime refuses the
    launch (GSL_ERR_HIP) -- the pattern of tests/test_marshalling_cpu.py."""
    lib = _lib()
    from gsplatloc_amd._lib import ptr

    N, C = 100, 2
    z = torch.zeros
    m, q, s, V, K = z(N, 3), z(N, 4), z(N, 3), z(C, 4, 4), z(C, 3, 3)
    head, tail = (ptr(m), ptr(q), ptr(s), ptr(V), ptr(K)), (64, 48, 0.3, 0.01, 1e10, 0.0)
    ws_bytes = lib.gsl_project_packed_ws_bytes(C, N)
    ws, nnz = z(ws_bytes, dtype=torch.uint8), z(1, dtype=torch.int32)
    assert lib.gsl_project_packed_count(*head, C, N, *tail, ptr(nnz), ptr(ws), ws_bytes, None) == HIP
    ids, rad = z(8, dtype=torch.int64), z(8, dtype=torch.int32)
    assert lib.gsl_project_packed_fill(*head, C, N, *tail, 8, ptr(ids), ptr(ids), ptr(rad), ptr(z(8, 2)), ptr(z(8)),
                                       ptr(z(8, 3)), ptr(z(8)), ptr(ws), ws_bytes, None) == HIP
    bws_bytes = lib.gsl_project_packed_bwd_ws_bytes(8, C)
    bws = z(bws_bytes, dtype=torch.uint8)
    for sparse, rows in ((0, N), (1, 8)):
        assert lib.gsl_project_packed_bwd(*head, C, N, 64, 48, 0.3, 8, ptr(ids), ptr(ids), ptr(z(8, 3)), ptr(z(8)),
                                          ptr(z(8, 2)), ptr(z(8)), ptr(z(8, 3)), ptr(z(8)), sparse, ptr(z(rows, 3)),
                                          ptr(z(rows, 4)), ptr(z(rows, 3)), ptr(z(C, 4, 4)), ptr(bws), bws_bytes,
                                          None) == HIP
    src, dst = z(N, 3), z(8, 3)
    assert lib.gsl_gather_rows(ptr(src), N, 3, ptr(ids), 8, ptr(dst), None) == HIP
    for unique in (0, 1):
        assert lib.gsl_scatter_add_rows(ptr(dst), ptr(ids), 8, 3, N, unique, ptr(src), None) == HIP


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_packed_ops_fail_loudly_without_gpu_tensors():
    """packed=True reaches the operators' own device check (there is no CPU path), not a NotImplementedError;
    sparse_grad without packed keeps raising."""
    import gsplatloc_amd as A

    m, q, s = torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4, 3)
    V, K = torch.eye(4)[None], torch.eye(3)[None]
    with pytest.raises(AssertionError, match="no CPU path"):
        A.fully_fused_projection(m, None, q, s, V, K, 32, 32, packed=True)
    with pytest.raises(AssertionError, match="no CPU path"):
        A.fully_fused_projection(m, None, q, s, V, K, 32, 32, packed=True, sparse_grad=True)
    with pytest.raises(NotImplementedError, match="sparse_grad requires packed=True"):
        A.fully_fused_projection(m, None, q, s, V, K, 32, 32, packed=False, sparse_grad=True)
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(AssertionError, match="no CPU path"):
        A.isect_tiles(torch.zeros(3, 2), torch.ones(3, dtype=torch.int32), torch.ones(3), 16, 2, 2, packed=True,
                      n_cameras=1, camera_ids=ids, gaussian_ids=ids)
    with pytest.raises(AssertionError, match="no CPU path"):
        A.rasterize_to_pixels(torch.zeros(3, 2), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3), 32, 32, 16,
                              torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), packed=True)
    with pytest.raises(NotImplementedError, match="masks"):
        A.rasterize_to_pixels(torch.zeros(3, 2), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3), 32, 32, 16,
                              torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), packed=True,
                              masks=torch.ones(1, 2, 2, dtype=torch.bool))
    from gsplatloc_amd.ops import gather_rows

    with pytest.raises(AssertionError, match="no CPU path"):
        gather_rows(m, ids)
    with pytest.raises(AssertionError, match="sparse_grad requires packed=True"):
        A.rasterization(m, q, s, torch.zeros(4), torch.zeros(4, 3), V, K, 32, 32, packed=False, sparse_grad=True)
    with pytest.raises(AssertionError, match="no CPU path"):
        A.rasterization(m, q, s, torch.zeros(4), torch.zeros(4, 3), V, K, 32, 32, packed=True, sparse_grad=True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_packed_projection_kernels_stay_in_registers():
    """ScratchSize 0 for every kernel of csrc/project_packed.hip: both passes of the forward, the three instances of
    the backward, the per-camera reduction -- and for the scan between the two passes, in csrc/compact.hip (register
    counts and occupancy: DESIGN.md section 4)."""
    res = {k: v for k, v in _resources("project_packed.hip").items() if "k_packed" in k}
    assert sum("k_packed_projectILb" in k for k in res) == 2
    assert sum("k_packed_project_bwd" in k for k in res) == 3
    assert sum("k_packed_reduce_viewmat" in k for k in res) == 1
    scan = {k: v for k, v in _resources("compact.hip").items() if "k_count_scan" in k}
    assert len(scan) == 1
    res.update(scan)
    rows = {k: v for k, v in _resources("project_packed.hip").items() if "k_gather_rows" in k or "k_scatter_" in k}
    assert len(rows) == 3  # the gather, its vjp with unique and with repeated ids
    res.update(rows)
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
