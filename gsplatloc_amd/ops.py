"""Stage operators with the gsplat 1.3.0 signatures, backed by libgsloc_hip.

Mirrors ``gsplat/cuda/_wrapper.py`` of the gsplat fork GsplatLoc installs
(un-vendored; signatures from /root/reference/.vscode/PythonImportHelper-v2-Completion.json):
``fully_fused_projection`` (IDX:14351), ``isect_tiles`` (IDX:14360),
``isect_offset_encode`` (IDX:14369), ``rasterize_to_pixels`` (IDX:14378),
``spherical_harmonics`` (IDX:14306).  Same argument names, shapes, return
tuples and assertion-style error behaviour; tensors are fp32 on the HIP device.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import check, current_stream, load_library, ptr

SUPPORTED_CHANNELS = (1, 2, 3, 4, 5, 8, 16, 32)


def _dev_f32(t: Tensor, name: str) -> Tensor:
    assert t.is_cuda, f"{name} must live on the GPU (got {t.device}); there is no CPU path"
    assert t.dtype == torch.float32, f"{name} must be float32 (got {t.dtype})"
    return t.contiguous()


# --------------------------------------------------------------------------- #
# projection
# --------------------------------------------------------------------------- #
class _FullyFusedProjection(torch.autograd.Function):
    """Projects Gaussians to 2D (autograd twin of gsplat's, IDX:14270)."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
                radius_clip, calc_compensations):
        lib = load_library()
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        radii = torch.empty(C, N, dtype=torch.int32, device=dev)
        means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(C, N, dtype=torch.float32, device=dev)
        conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
        comps = torch.empty(C, N, dtype=torch.float32, device=dev) if calc_compensations else None
        st = current_stream()
        for c in range(C):
            check(lib.gsl_project_fwd(ptr(means), ptr(quats), ptr(scales), ptr(viewmats[c]), ptr(Ks[c]), N, width,
                                      height, eps2d, near_plane, far_plane, radius_clip, ptr(radii[c]),
                                      ptr(means2d[c]), ptr(depths[c]), ptr(conics[c]),
                                      ptr(comps[c]) if comps is not None else None, st), "gsl_project_fwd")
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii, conics,
                              comps if comps is not None else torch.empty(0, device=dev))
        ctx.dims = (width, height, eps2d, calc_compensations)
        ctx.mark_non_differentiable(radii)
        if comps is None:
            return radii, means2d, depths, conics, None
        return radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, v_radii, v_means2d, v_depths, v_conics, v_comps):
        lib = load_library()
        means, quats, scales, viewmats, Ks, radii, conics, comps = ctx.saved_tensors
        width, height, eps2d, calc_comp = ctx.dims
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        need_full = any(ctx.needs_input_grad[:3])
        need_view = ctx.needs_input_grad[3]
        v_means2d = v_means2d.contiguous()
        v_depths = v_depths.contiguous()
        v_conics = v_conics.contiguous()
        if calc_comp and v_comps is not None:
            v_comps = v_comps.contiguous()
        else:
            v_comps = None
        v_means = v_quats = v_scales = None
        v_viewmats = torch.zeros(C, 4, 4, dtype=torch.float32, device=dev) if need_view else None
        ws_bytes = lib.gsl_project_bwd_ws_bytes(N)
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        st = current_stream()
        for c in range(C):
            if need_full:
                vm = torch.empty(N, 3, dtype=torch.float32, device=dev)
                vq = torch.empty(N, 4, dtype=torch.float32, device=dev)
                vs = torch.empty(N, 3, dtype=torch.float32, device=dev)
            else:
                vm = vq = vs = None
            check(lib.gsl_project_bwd(
                ptr(means), ptr(quats), ptr(scales), ptr(viewmats[c]), ptr(Ks[c]), N, width, height, eps2d,
                ptr(radii[c]), ptr(conics[c]), ptr(comps[c]) if calc_comp else None, ptr(v_means2d[c]),
                ptr(v_depths[c]), ptr(v_conics[c]), ptr(v_comps[c]) if v_comps is not None else None, ptr(vm),
                ptr(vq), ptr(vs), ptr(v_viewmats[c]) if need_view else None, ptr(ws), ws_bytes, st),
                "gsl_project_bwd")
            if need_full:
                v_means = vm if v_means is None else v_means + vm
                v_quats = vq if v_quats is None else v_quats + vq
                v_scales = vs if v_scales is None else v_scales + vs
        ni = ctx.needs_input_grad
        return (v_means if ni[0] else None, v_quats if ni[1] else None, v_scales if ni[2] else None,
                v_viewmats, None, None, None, None, None, None, None, None)


class _PackedProjection(torch.autograd.Function):
    """Packed projection: one row per (camera, Gaussian) pair with radii > 0, in camera-major order
    (csrc/project_packed.hip).  With ``sparse_grad`` the gradients of means / quats / scales are sparse COO tensors
    over the visible rows."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip,
                calc_compensations, sparse_grad):
        lib = load_library()
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        st = current_stream()
        ws_bytes = lib.gsl_project_packed_ws_bytes(C, N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        nnz_dev = torch.empty(1, dtype=torch.int32, device=dev)
        args = (ptr(means), ptr(quats), ptr(scales), ptr(viewmats), ptr(Ks), C, N, width, height, eps2d, near_plane,
                far_plane, radius_clip)
        check(lib.gsl_project_packed_count(*args, ptr(nnz_dev), ptr(ws), ws_bytes, st), "gsl_project_packed_count")
        nnz = int(nnz_dev.item())  # host sync: output sizes depend on it (as in gsplat)
        camera_ids = torch.empty(nnz, dtype=torch.int64, device=dev)
        gaussian_ids = torch.empty(nnz, dtype=torch.int64, device=dev)
        radii = torch.empty(nnz, dtype=torch.int32, device=dev)
        means2d = torch.empty(nnz, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(nnz, dtype=torch.float32, device=dev)
        conics = torch.empty(nnz, 3, dtype=torch.float32, device=dev)
        comps = torch.empty(nnz, dtype=torch.float32, device=dev) if calc_compensations else None
        check(lib.gsl_project_packed_fill(*args, nnz, ptr(camera_ids), ptr(gaussian_ids), ptr(radii), ptr(means2d),
                                          ptr(depths), ptr(conics), ptr(comps), ptr(ws), ws_bytes, st),
              "gsl_project_packed_fill")
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, camera_ids, gaussian_ids, conics,
                              comps if comps is not None else torch.empty(0, device=dev))
        ctx.dims = (width, height, eps2d, calc_compensations, sparse_grad)
        ctx.mark_non_differentiable(camera_ids, gaussian_ids, radii)
        return camera_ids, gaussian_ids, radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, v_camera_ids, v_gaussian_ids, v_radii, v_means2d, v_depths, v_conics, v_comps):
        lib = load_library()
        means, quats, scales, viewmats, Ks, camera_ids, gaussian_ids, conics, comps = ctx.saved_tensors
        width, height, eps2d, calc_comp, sparse_grad = ctx.dims
        C, N = viewmats.shape[0], means.shape[0]
        nnz = camera_ids.numel()
        dev = means.device
        ni = ctx.needs_input_grad
        need_full = any(ni[:3])
        v_means2d, v_depths, v_conics = v_means2d.contiguous(), v_depths.contiguous(), v_conics.contiguous()
        v_comps = v_comps.contiguous() if (calc_comp and v_comps is not None) else None
        v_means = v_quats = v_scales = None
        if need_full:
            rows = nnz if sparse_grad else N
            v_means = torch.empty(rows, 3, dtype=torch.float32, device=dev)
            v_quats = torch.empty(rows, 4, dtype=torch.float32, device=dev)
            v_scales = torch.empty(rows, 3, dtype=torch.float32, device=dev)
        v_viewmats = torch.empty(C, 4, 4, dtype=torch.float32, device=dev) if ni[3] else None
        ws_bytes = lib.gsl_project_packed_bwd_ws_bytes(nnz, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.gsl_project_packed_bwd(
            ptr(means), ptr(quats), ptr(scales), ptr(viewmats), ptr(Ks), C, N, width, height, eps2d, nnz,
            ptr(camera_ids), ptr(gaussian_ids), ptr(conics), ptr(comps) if calc_comp else None, ptr(v_means2d),
            ptr(v_depths), ptr(v_conics), ptr(v_comps), int(sparse_grad), ptr(v_means), ptr(v_quats), ptr(v_scales),
            ptr(v_viewmats), ptr(ws), ws_bytes, current_stream()), "gsl_project_packed_bwd")
        if need_full and sparse_grad:
            # a Gaussian has one row per camera that sees it: the indices are unique (coalesced) for one camera only
            idx = gaussian_ids[None]
            v_means = torch.sparse_coo_tensor(idx, v_means, size=means.shape, is_coalesced=(C == 1))
            v_quats = torch.sparse_coo_tensor(idx, v_quats, size=quats.shape, is_coalesced=(C == 1))
            v_scales = torch.sparse_coo_tensor(idx, v_scales, size=scales.shape, is_coalesced=(C == 1))
            if C == 1:
                # autograd takes a sparse gradient nobody else holds by a shallow copy that forgets the coalesced
                # flag; a second reference makes it clone the tensor, and the clone keeps the flag
                ctx.coalesced_grads = (v_means, v_quats, v_scales)
        return (v_means if ni[0] else None, v_quats if ni[1] else None, v_scales if ni[2] else None, v_viewmats,
                None, None, None, None, None, None, None, None, None)


class _GatherRows(torch.autograd.Function):
    """src[ids] for the packed rows and its vjp on the HIP kernels (torch's indexing backward serialises on repeated
    indices: a third of a second for a million rows of one camera's position)."""

    @staticmethod
    def forward(ctx, src, ids, unique):
        lib = load_library()
        n_src, nnz = src.shape[0], ids.numel()
        D = int(math.prod(src.shape[1:]))  # floats per row
        dst = torch.empty((nnz,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
        if D:
            check(lib.gsl_gather_rows(ptr(src), n_src, D, ptr(ids), nnz, ptr(dst), current_stream()), "gsl_gather_rows")
        ctx.save_for_backward(ids)
        ctx.meta = (tuple(src.shape), D, unique)
        return dst

    @staticmethod
    def backward(ctx, v_rows):
        lib = load_library()
        (ids,) = ctx.saved_tensors
        shape, D, unique = ctx.meta
        v_src = torch.empty(shape, dtype=torch.float32, device=v_rows.device)
        if D:
            check(lib.gsl_scatter_add_rows(ptr(v_rows.contiguous()), ptr(ids), ids.numel(), D, shape[0], int(unique),
                                           ptr(v_src), current_stream()), "gsl_scatter_add_rows")
        return v_src, None, None


def gather_rows(src: Tensor, ids: Tensor, unique: bool = False) -> Tensor:
    """``src[ids]`` for int64 ``ids`` [nnz] and float32 ``src`` [n, ...] on the device: the rows a packed pipeline
    needs of a per-Gaussian (``gaussian_ids``) or per-camera (``camera_ids``) tensor.  ``unique``: no id occurs twice
    (one camera's ``gaussian_ids``), the backward then stores instead of adding atomically."""
    assert ids.dim() == 1 and ids.dtype == torch.int64, (ids.shape, ids.dtype)
    assert src.dim() >= 1 and src.shape[0] < 2 ** 31, src.shape
    return _GatherRows.apply(_dev_f32(src, "src"), ids.contiguous(), bool(unique))


def fully_fused_projection(
    means: Tensor,  # [N, 3]
    covars: Optional[Tensor],  # [N, 6] or None
    quats: Optional[Tensor],  # [N, 4] or None
    scales: Optional[Tensor],  # [N, 3] or None
    viewmats: Tensor,  # [C, 4, 4]
    Ks: Tensor,  # [C, 3, 3]
    width: int,
    height: int,
    eps2d: float = 0.3,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    packed: bool = False,
    sparse_grad: bool = False,
    calc_compensations: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor]]:
    """Project Gaussians to the image plane: radii [C,N] int32, means2d [C,N,2],
    depths [C,N], conics [C,N,3], compensations [C,N] | None.

    ``packed=True`` returns (camera_ids [nnz] int64, gaussian_ids [nnz] int64, radii [nnz], means2d [nnz,2],
    depths [nnz], conics [nnz,3], compensations [nnz] | None): one row per (camera, Gaussian) pair with radii > 0, in
    ascending order of camera * N + gaussian, each row holding the bits of the dense call's.  With ``sparse_grad`` (packed
    only) the gradients of means / quats / scales are sparse COO tensors indexed by ``gaussian_ids`` (coalesced for one
    camera); the gradient of viewmats stays dense."""
    C = viewmats.size(0)
    N = means.size(0)
    assert means.size() == (N, 3), means.size()
    assert viewmats.size() == (C, 4, 4), viewmats.size()
    assert Ks.size() == (C, 3, 3), Ks.size()
    if covars is not None:
        raise NotImplementedError("precomputed covars are not supported; pass quats and scales (as GsplatLoc does)")
    assert quats is not None, "covars or quats is required"
    assert scales is not None, "covars or scales is required"
    assert quats.size() == (N, 4), quats.size()
    assert scales.size() == (N, 3), scales.size()
    if sparse_grad and not packed:
        raise NotImplementedError("sparse_grad requires packed=True")
    means, quats, scales = _dev_f32(means, "means"), _dev_f32(quats, "quats"), _dev_f32(scales, "scales")
    viewmats, Ks = _dev_f32(viewmats, "viewmats"), _dev_f32(Ks, "Ks")
    if packed:
        return _PackedProjection.apply(means, quats, scales, viewmats, Ks, int(width), int(height), float(eps2d),
                                       float(near_plane), float(far_plane), float(radius_clip),
                                       bool(calc_compensations), bool(sparse_grad))
    return _FullyFusedProjection.apply(means, quats, scales, viewmats, Ks, int(width), int(height), float(eps2d),
                                       float(near_plane), float(far_plane), float(radius_clip),
                                       bool(calc_compensations))


# --------------------------------------------------------------------------- #
# spherical harmonics
# --------------------------------------------------------------------------- #
class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degree, dirs, coeffs, masks):
        lib = load_library()
        M = dirs.numel() // 3
        K = coeffs.shape[-2]
        colors = torch.empty(dirs.shape, dtype=torch.float32, device=dirs.device)
        check(lib.gsl_sh_fwd(degree, ptr(dirs), ptr(coeffs), ptr(masks), M, K, ptr(colors), current_stream()),
              "gsl_sh_fwd")
        ctx.save_for_backward(dirs, coeffs, masks if masks is not None else torch.empty(0, device=dirs.device))
        ctx.meta = (degree, M, K, masks is not None)
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        lib = load_library()
        dirs, coeffs, masks = ctx.saved_tensors
        degree, M, K, has_mask = ctx.meta
        v_colors = v_colors.contiguous()
        v_coeffs = torch.empty_like(coeffs)
        v_dirs = torch.empty_like(dirs) if ctx.needs_input_grad[1] else None
        check(lib.gsl_sh_bwd(degree, ptr(dirs), ptr(coeffs), ptr(masks) if has_mask else None, M, K, ptr(v_colors),
                             ptr(v_coeffs), ptr(v_dirs), current_stream()), "gsl_sh_bwd")
        return None, v_dirs, v_coeffs if ctx.needs_input_grad[2] else None, None


def spherical_harmonics(degrees_to_use: int, dirs: Tensor, coeffs: Tensor, masks: Optional[Tensor] = None) -> Tensor:
    """Colours [...,3] from SH coefficients [...,K,3] along (unnormalised) dirs [...,3]."""
    assert 0 <= degrees_to_use <= 3, "SH degree 0..3 is supported"
    assert (degrees_to_use + 1) ** 2 <= coeffs.shape[-2], coeffs.shape
    assert dirs.shape[:-1] == coeffs.shape[:-2], (dirs.shape, coeffs.shape)
    assert dirs.shape[-1] == 3, dirs.shape
    assert coeffs.shape[-1] == 3, coeffs.shape
    if masks is not None:
        assert masks.shape == dirs.shape[:-1], masks.shape
        masks = masks.to(torch.bool).contiguous().view(torch.uint8)
    return _SphericalHarmonics.apply(int(degrees_to_use), _dev_f32(dirs, "dirs"), _dev_f32(coeffs, "coeffs"), masks)


# --------------------------------------------------------------------------- #
# tile binning
# --------------------------------------------------------------------------- #
def tile_n_bits(n_tiles: int) -> int:
    return int(math.floor(math.log2(n_tiles))) + 1


@torch.no_grad()
def isect_tiles(
    means2d: Tensor,  # [C, N, 2]
    radii: Tensor,  # [C, N]
    depths: Tensor,  # [C, N]
    tile_size: int,
    tile_width: int,
    tile_height: int,
    sort: bool = True,
    packed: bool = False,
    n_cameras: Optional[int] = None,
    camera_ids: Optional[Tensor] = None,
    gaussian_ids: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Tensor]:
    """Map projected Gaussians to intersecting tiles.

    Returns tiles_per_gauss [C,N] int32, isect_ids [I] int64 (camera | tile | depth bits),
    flatten_ids [I] int32 (index into the flattened [C*N] arrays); sorted by isect_ids when
    ``sort`` (ties in Gaussian-index order, as a stable sort of the emit order gives).

    ``packed=True``: means2d [nnz,2], radii [nnz], depths [nnz] are the rows of the packed projection (sorted by
    camera; ``n_cameras``, ``camera_ids``, ``gaussian_ids`` are required), tiles_per_gauss is [nnz] and flatten_ids
    index the packed rows.

    With ``sort``, every Gaussian with radii > 0 must have a depth from +0.0 to +inf (sign bit clear, not NaN):
    the per-tile sorts compare (depth bits, id) keys partly as doubles and partly as unsigned integers, which agree
    only there (include/gsloc_hip.h, gsl_tile_sort).  Anything else raises ValueError.  The projection culls z <= near,
    so its outputs always qualify."""
    if packed:
        nnz = means2d.shape[0]
        assert means2d.shape == (nnz, 2), means2d.size()
        assert radii.shape == (nnz,), radii.size()
        assert depths.shape == (nnz,), depths.size()
        assert n_cameras is not None, "n_cameras is required if packed is True"
        assert camera_ids is not None and camera_ids.shape == (nnz,), "camera_ids [nnz] is required if packed is True"
        assert gaussian_ids is not None and gaussian_ids.shape == (nnz,), "gaussian_ids [nnz] is required if packed is True"
        C = int(n_cameras)
    else:
        C, N, _ = means2d.shape
        assert means2d.shape == (C, N, 2), means2d.size()
        assert radii.shape == (C, N), radii.size()
        assert depths.shape == (C, N), depths.size()
    lib = load_library()
    dev = means2d.device
    means2d, depths = _dev_f32(means2d, "means2d"), _dev_f32(depths, "depths")
    radii = radii.to(torch.int32).contiguous()
    if packed:
        # camera c's rows are one contiguous slice (the rows are sorted by camera): the per-camera kernels run on the
        # slices, the slice start is the id offset
        bounds = torch.searchsorted(camera_ids.contiguous(), torch.arange(C + 1, device=dev)).tolist()  # host sync
        spans = [(bounds[c], bounds[c + 1] - bounds[c]) for c in range(C)]
        out_shape = (nnz,)
    else:
        spans = [(c * N, N) for c in range(C)]
        out_shape = (C, N)
        means2d, depths, radii = means2d.view(C * N, 2), depths.view(C * N), radii.view(C * N)
    n_tiles = tile_width * tile_height
    nbits = tile_n_bits(n_tiles)
    st = current_stream()
    tiles_per_gauss = torch.empty(radii.shape[0], dtype=torch.int32, device=dev)
    ws_bytes = lib.gsl_isect_ws_bytes(n_tiles)
    wss = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(C)]
    offs = torch.empty(C, n_tiles + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(C, dtype=torch.int32, device=dev)

    def rows(t, c):  # pointer to camera c's first row (NULL for a camera without rows)
        lo, n = spans[c]
        return ptr(t[lo:]) if n else None

    for c in range(C):
        check(lib.gsl_isect_count(rows(means2d, c), rows(radii, c), spans[c][1], tile_size, tile_width, tile_height, 0,
                                  tile_height, rows(tiles_per_gauss, c), ptr(offs[c]), ptr(counts[c:c + 1]),
                                  ptr(wss[c]), ws_bytes, st), "gsl_isect_count")
    tiles_per_gauss = tiles_per_gauss.view(out_shape)
    if sort:
        # visible Gaussians whose depth the sort cannot order: sign bit set (negative, -0.0) or NaN (> +inf's bits)
        bits = depths.view(torch.int32)
        bad = ((radii > 0) & ((bits < 0) | (bits > 0x7F800000))).sum(dtype=torch.int32).view(1)
        per_cam = torch.cat([counts, bad]).tolist()  # host sync: output sizes depend on it (as in gsplat)
        if per_cam.pop():
            raise ValueError("isect_tiles: a Gaussian with radii > 0 has a negative, -0.0 or NaN depth; the tile sort "
                             "orders depths from +0.0 to +inf only")
    else:
        per_cam = counts.tolist()  # host sync: output sizes depend on it (as in gsplat)
    total = int(sum(per_cam))
    isect_ids = torch.empty(total, dtype=torch.int64, device=dev)
    flatten_ids = torch.empty(total, dtype=torch.int32, device=dev)
    if total == 0:
        return tiles_per_gauss, isect_ids, flatten_ids
    base = 0
    if sort:
        keys = torch.empty(max(per_cam), dtype=torch.int64, device=dev)
        for c in range(C):
            n = per_cam[c]
            if n:
                check(lib.gsl_isect_fill(rows(means2d, c), rows(radii, c), rows(depths, c), spans[c][1], tile_size,
                                         tile_width, tile_height, 0, tile_height, c, nbits, ptr(offs[c]), n, ptr(keys),
                                         ptr(flatten_ids[base:]), ptr(isect_ids[base:]), ptr(wss[c]), ws_bytes, st),
                      "gsl_isect_fill")
                if spans[c][0]:
                    flatten_ids[base:base + n] += spans[c][0]
            base += n
    else:
        for c in range(C):
            n = per_cam[c]
            if n:
                lo, m = spans[c]
                cum = torch.cumsum(tiles_per_gauss.view(-1)[lo:lo + m].to(torch.int64), dim=0)
                check(lib.gsl_isect_emit(rows(means2d, c), rows(radii, c), rows(depths, c), ptr(cum), m, tile_size,
                                         tile_width, tile_height, c, nbits, lo, ptr(isect_ids[base:]),
                                         ptr(flatten_ids[base:]), st), "gsl_isect_emit")
            base += n
    return tiles_per_gauss, isect_ids, flatten_ids


@torch.no_grad()
def isect_offset_encode(isect_ids: Tensor, n_cameras: int, tile_width: int, tile_height: int) -> Tensor:
    """Start offset of every (camera, tile) in the sorted intersection list: [C, tile_height, tile_width] int32."""
    lib = load_library()
    n_tiles = tile_width * tile_height
    offsets = torch.empty(n_cameras, tile_height, tile_width, dtype=torch.int32, device=isect_ids.device)
    isect_ids = isect_ids.contiguous()
    check(lib.gsl_isect_offsets(ptr(isect_ids) if isect_ids.numel() else None, isect_ids.numel(), n_cameras, n_tiles,
                                tile_n_bits(n_tiles), ptr(offsets), current_stream()), "gsl_isect_offsets")
    return offsets


# --------------------------------------------------------------------------- #
# compositing
# --------------------------------------------------------------------------- #
def _pad_channels(D: int) -> int:
    for s in SUPPORTED_CHANNELS:
        if D <= s:
            return s
    raise AssertionError(f"Unsupported number of color channels: {D} (max {SUPPORTED_CHANNELS[-1]})")


class _RasterizeToPixels(torch.autograd.Function):
    """Rasterize gaussians (autograd twin of gsplat's, IDX:14279)."""

    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, backgrounds, width, height, tile_size, isect_offsets,
                flatten_ids, absgrad=False):
        lib = load_library()
        D = colors.shape[-1]  # per-Gaussian arrays: [C,N,.] or, packed, [nnz,.]; flatten_ids index their rows
        C, th, tw = isect_offsets.shape
        dev = means2d.device
        n_tiles = th * tw
        n_isects = flatten_ids.numel()
        offs_ext = torch.cat([isect_offsets.reshape(-1).to(torch.int32),
                              torch.tensor([n_isects], dtype=torch.int32, device=dev)]).contiguous()
        render_colors = torch.empty(C, height, width, D, dtype=torch.float32, device=dev)
        render_alphas = torch.empty(C, height, width, 1, dtype=torch.float32, device=dev)
        last_ids = torch.empty(C, height, width, dtype=torch.int32, device=dev)
        # the transmittance every pixel ends with, for the backward: 1 - render_alphas keeps 2^-24 absolute of it, which
        # behind many thin layers (T near the 1e-4 stop) is 3e-4 relative -- of every gradient term of the pixel
        t_final = torch.empty(C, height, width, dtype=torch.float32, device=dev)
        st = current_stream()
        for c in range(C):
            check(lib.gsl_rasterize_fwd(
                ptr(means2d), ptr(conics), ptr(colors), ptr(opacities),
                ptr(backgrounds[c]) if backgrounds is not None else None, D, width, height, tile_size, tw, th, 0, th,
                ptr(offs_ext[c * n_tiles:]), ptr(flatten_ids) if n_isects else None, n_isects, ptr(render_colors[c]),
                ptr(render_alphas[c]), ptr(last_ids[c]), ptr(t_final[c]), st), "gsl_rasterize_fwd")
        ctx.save_for_backward(means2d, conics, colors, opacities,
                              backgrounds if backgrounds is not None else torch.empty(0, device=dev), offs_ext,
                              flatten_ids, render_alphas, last_ids, t_final)
        ctx.dims = (width, height, tile_size, tw, th, C, backgrounds is not None)
        ctx.absgrad = absgrad
        return render_colors, render_alphas

    @staticmethod
    def backward(ctx, v_render_colors, v_render_alphas):
        lib = load_library()
        (means2d, conics, colors, opacities, backgrounds, offs_ext, flatten_ids, render_alphas,
         last_ids, t_final) = ctx.saved_tensors
        width, height, tile_size, tw, th, C, has_bg = ctx.dims
        D = colors.shape[-1]
        n_rows = opacities.numel()
        n_tiles = th * tw
        n_isects = flatten_ids.numel()
        v_render_colors = v_render_colors.contiguous()
        v_render_alphas = v_render_alphas.contiguous()
        v_means2d = torch.empty_like(means2d)
        v_conics = torch.empty_like(conics)
        v_colors = torch.empty_like(colors)
        v_opacities = torch.empty_like(opacities)
        st = current_stream()
        vacc = torch.zeros(lib.gsl_vacc_bytes(n_rows, D) // 4, dtype=torch.float32, device=means2d.device)
        if n_isects:
            for c in range(C):
                check(lib.gsl_rasterize_bwd(
                    ptr(means2d), ptr(conics), ptr(colors), ptr(opacities), ptr(backgrounds[c]) if has_bg else None,
                    D, width, height, tile_size, tw, th, 0, th, ptr(offs_ext[c * n_tiles:]), ptr(flatten_ids),
                    n_isects, ptr(render_alphas[c]), ptr(last_ids[c]), ptr(t_final[c]), ptr(v_render_colors[c]),
                    ptr(v_render_alphas[c]), ptr(vacc), st), "gsl_rasterize_bwd")
        check(lib.gsl_vacc_unpack(ptr(vacc), n_rows, D, ptr(v_means2d), ptr(v_conics), ptr(v_colors),
                                  ptr(v_opacities), st), "gsl_vacc_unpack")
        if ctx.absgrad:
            # sum over pixels of |per-pixel v_means2d| (gsplat's means2d.absgrad), set on the caller's means2d: the
            # compositing backward's sums cannot give it (|.| of a sum), csrc/absgrad.hip walks the pixels once more
            absgrad = torch.zeros_like(means2d)
            for c in range(C):
                check(lib.gsl_rasterize_absgrad(
                    ptr(means2d), ptr(conics), ptr(colors), ptr(opacities), ptr(backgrounds[c]) if has_bg else None,
                    D, width, height, tile_size, tw, th, ptr(offs_ext[c * n_tiles:]),
                    ptr(flatten_ids) if n_isects else None, n_isects, ptr(render_alphas[c]), ptr(last_ids[c]),
                    ptr(t_final[c]), ptr(v_render_colors[c]), ptr(v_render_alphas[c]), ptr(absgrad), st),
                    "gsl_rasterize_absgrad")
            means2d.absgrad = absgrad  # assigned by every backward, as gsplat does
        v_backgrounds = None
        if has_bg and ctx.needs_input_grad[4]:
            v_backgrounds = (v_render_colors * t_final[..., None]).sum(dim=(1, 2))
        return v_means2d, v_conics, v_colors, v_opacities, v_backgrounds, None, None, None, None, None, None


def rasterize_to_pixels(
    means2d: Tensor,  # [C, N, 2]
    conics: Tensor,  # [C, N, 3]
    colors: Tensor,  # [C, N, channels]
    opacities: Tensor,  # [C, N]
    image_width: int,
    image_height: int,
    tile_size: int,
    isect_offsets: Tensor,  # [C, tile_height, tile_width]
    flatten_ids: Tensor,  # [n_isects]
    backgrounds: Optional[Tensor] = None,  # [C, channels]
    masks: Optional[Tensor] = None,
    packed: bool = False,
    absgrad: bool = False,
) -> Tuple[Tensor, Tensor]:
    """Rasterize to pixels: render_colors [C,H,W,channels], render_alphas [C,H,W,1].

    ``absgrad``: the backward also sets ``means2d.absgrad`` [C,N,2], the per-component sum over pixels of
    |d L_p / d means2d| (gsplat's densification statistic).

    ``packed=True``: means2d [nnz,2], conics [nnz,3], colors [nnz,channels], opacities [nnz] are packed rows and
    flatten_ids index them; ``means2d.absgrad`` is then [nnz,2]."""
    if masks is not None:
        raise NotImplementedError("tile masks are not supported")
    C = isect_offsets.size(0)
    if packed:
        nnz = means2d.size(0)
        assert means2d.shape == (nnz, 2), means2d.shape
        assert conics.shape == (nnz, 3), conics.shape
        assert colors.shape[0] == nnz and colors.dim() == 2, colors.shape
        assert opacities.shape == (nnz,), opacities.shape
    else:
        N = means2d.size(1)
        assert means2d.shape == (C, N, 2), means2d.shape
        assert conics.shape == (C, N, 3), conics.shape
        assert colors.shape[:2] == (C, N), colors.shape
        assert opacities.shape == (C, N), opacities.shape
    if backgrounds is not None:
        assert backgrounds.shape == (C, colors.shape[-1]), backgrounds.shape
        backgrounds = _dev_f32(backgrounds, "backgrounds")
    assert tile_size == 16, "the gfx950 kernels are built for 16x16 tiles (gsplat's default)"
    tile_height, tile_width = isect_offsets.shape[1:3]
    assert tile_height * tile_size >= image_height, f"Assert Failed: {tile_height} * {tile_size} >= {image_height}"
    assert tile_width * tile_size >= image_width, f"Assert Failed: {tile_width} * {tile_size} >= {image_width}"
    channels = colors.shape[-1]
    padded = _pad_channels(channels)
    if padded != channels:
        colors = torch.cat([colors, torch.zeros(*colors.shape[:-1], padded - channels, device=colors.device,
                                                dtype=colors.dtype)], dim=-1)
        if backgrounds is not None:
            backgrounds = torch.cat([backgrounds, torch.zeros(C, padded - channels, device=colors.device,
                                                              dtype=colors.dtype)], dim=-1)
    render_colors, render_alphas = _RasterizeToPixels.apply(
        _dev_f32(means2d, "means2d"), _dev_f32(conics, "conics"), _dev_f32(colors, "colors"),
        _dev_f32(opacities, "opacities"), backgrounds, int(image_width), int(image_height), int(tile_size),
        isect_offsets.contiguous(), flatten_ids.to(torch.int32).contiguous(), bool(absgrad))
    if padded != channels:
        render_colors = render_colors[..., :channels]
    return render_colors, render_alphas
