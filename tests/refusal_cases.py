"""Calls that the entry points of the pipeline files (csrc/cl_tiles, cl_seg_loss, cl_surface_dist, cl_conn_comp, cl_resample, cl_spline,
cl_augment, cl_preprocess, cl_zoom2d) refuse before any launch, and the status each must return.  The statuses are RECORDED
(tests/golden/refusal_codes.json, tests/golden/make_golden_refusals.py): what the commit before the shared storage / extent / dispatch header
returned, including which of two bad fields is reported first.  Every case has at least one bad field; no buffer is ever read."""
import ctypes
import json
import os

from deformablelka_amd import _lib as L

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_codes.json")

_BUF = [ctypes.create_string_buffer(256) for _ in range(2)]
P, Q = (ctypes.addressof(b) for b in _BUF)      # two distinct, 16-byte aligned enough, never dereferenced
LIM = 0x7fffffff
i3 = ctypes.c_int64 * 3
ci = ctypes.c_int * 8


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _desc(cls, base, **kw):
    d = cls()
    for k, v in {**base, **kw}.items():
        if isinstance(v, (tuple, list)):
            arr = getattr(d, k)
            for j, x in enumerate(v):
                arr[j] = x
        else:
            setattr(d, k, v)
    return ctypes.byref(d)


def zm(**kw):
    return _desc(L.Zoom2dDesc, dict(in_dtype=L.DLKA_F32, out_dtype=L.DLKA_F32, taps=2, normalize=0, N=1, in_=(4, 4), out=(4, 4), mean=0., std=1.), **kw)


def rs(**kw):
    return _desc(L.ResampleDesc, dict(C=1, dtype=L.DLKA_F32, taps=(1, 2, 2), in_=(3, 4, 5), out=(4, 5, 6)), **kw)


def ag(**kw):
    return _desc(L.AugmentDesc, dict(B=1, C=1, dtype=L.DLKA_F32, order=1, mode=L.DLKA_AUG_CONSTANT, pad=0, src=(3, 4, 5), out=(3, 4, 6), cval=0.),
                 **kw)


def ag2(**kw):
    return ag(**{**dict(src=(4, 5, 0), out=(4, 6, 0)), **kw})


def pp(**kw):
    return _desc(L.PrepDesc, dict(rank=3, C=1, seg_channels=0, nan_to_zero=0, nonzero_label=-1, ext=(3, 4, 5), lo=(0, 0, 0), hi=(3, 4, 5)), **kw)


def sd(**kw):
    return _desc(L.SurfaceDistDesc, dict(rank=3, connectivity=1, label_dtype=L.DLKA_SD_U8, K=1, mask_mode=0, ext=(3, 4, 5), spacing=(1., 1., 1.),
                                         class_id=(1,)), **kw)


def cc(**kw):
    return _desc(L.ConnCompDesc, dict(rank=3, connectivity=1, label_dtype=L.DLKA_SD_U8, K=1, mask_mode=0, n_ids=1, has_min=0, ext=(3, 4, 5),
                                      class_id=(1,), entry_of=(0,), min_count=(0,)), **kw)


def sl(**kw):
    return _desc(L.SegLossDesc, dict(B=1, K=2, N=8, dtype=L.DLKA_F32, label_dtype=L.DLKA_LABEL_F32, mode=L.DLKA_SEG_LOSS_NNUNET, batch_dice=0,
                                     do_bg=0, smooth=1e-5, weight_ce=1., weight_dice=1.), **kw)


BIG3 = (65536, 65536, 1)                        # 2^32 cells
ORG, MSK = ci(0, 0, 0), ci(0)                   # one tile at the origin, no mirroring


def _gather(x=P, C=1, X=4, Y=4, Z=4, org=ORG, T=1, msk=MSK, M=1, p=(2, 2, 2), pad=(0, 0, 0), out=Q):
    return ("dlka_tiles_gather", (x, C, X, Y, Z, org, T, msk, M) + tuple(p) + tuple(pad) + (0., out, None))


def _blend(x=P, dtype=L.DLKA_F32, K=2, nl=L.DLKA_TILES_SOFTMAX, score=Q, weight=Q, ext=(4, 4, 4), org=ORG, T=1, msk=MSK, M=1, p=(2, 2, 2)):
    return ("dlka_tiles_blend", (x, dtype, K, nl, 1., None, score, weight) + tuple(ext) + (org, T, msk, M) + tuple(p) + (None,))


def _final(score=P, K=2, ext=(4, 4, 4), pad=(0, 0, 0), keep=(4, 4, 4), probs=Q):
    return ("dlka_tiles_finalize", (score, P, K) + tuple(ext) + tuple(pad) + tuple(keep) + (probs, Q, None))


def _gauss(x=P, y=Q, dtype=L.DLKA_F32, ch=1, ext=(3, 4, 5), axis=0, radius=P):
    return ("dlka_augment_gaussian", (x, y, dtype, ch, i3(*ext) if ext else None, axis, radius, P, None))


def _stats(x=P, stats=Q, ws=Q, nbytes=256, dtype=L.DLKA_F32, ch=1, cells=8):
    return ("dlka_augment_channel_stats", (x, stats, ws, nbytes, dtype, ch, cells, None))


def _point(x=P, y=Q, dtype=L.DLKA_F32, B=1, C=1, ext=(3, 4, 5), ops=P):
    return ("dlka_augment_pointwise", (x, None, y, dtype, B, C, i3(*ext) if ext else None, ops, None, None, None, None))


def _pad(x=P, y=Q, dtype=L.DLKA_F32, n=(3, 4, 5), pad=(1, 1, 1)):
    return ("dlka_spline_pad", (x, y, dtype, i3(*n) if n else None, i3(*pad), None))


def _pre(c=P, ext=(3, 4, 5), axis=0, boundary=L.DLKA_SPLINE_MIRROR):
    return ("dlka_spline_prefilter", (c, i3(*ext) if ext else None, axis, boundary, None))


BOX = (ctypes.c_int64 * 6)
NO_WORK = ("sd_distances/empty_boxes", "cc_component_table/capacity_zero")   # nothing to do: DLKA_OK without a launch


def cases():
    """{id: (entry point, arguments)}; ids are "<entry>/<what is wrong>", two bad fields joined by '+' in the order of the argument list."""
    z, r, a, t = "dlka_zoom2d_", "dlka_resample_", "dlka_augment_", "dlka_prep_"
    over_aug = LIM - 127                        # one over the source limit of the augmentation (2^31 - 1 - 128)
    c = {
        # ---- cl_zoom2d ----
        "zoom2d_spline/null_desc": (z + "spline", (P, Q, None, P, P, None)),
        "zoom2d_spline/null_src": (z + "spline", (None, Q, zm(), P, P, None)),
        "zoom2d_spline/null_w4": (z + "spline", (P, Q, zm(), P, None, None)),
        "zoom2d_spline/N_zero": (z + "spline", (P, Q, zm(N=0), P, P, None)),
        "zoom2d_spline/in_zero": (z + "spline", (P, Q, zm(in_=(4, 0)), P, P, None)),
        "zoom2d_spline/in_over": (z + "spline", (P, Q, zm(in_=(0x40000000, 1)), P, P, None)),
        "zoom2d_spline/out_over": (z + "spline", (P, Q, zm(out=(1, 0x40000000)), P, P, None)),
        "zoom2d_spline/N_over": (z + "spline", (P, Q, zm(N=2 ** 31), P, P, None)),
        "zoom2d_spline/N_huge": (z + "spline", (P, Q, zm(N=2 ** 62), P, P, None)),
        "zoom2d_spline/cells_over": (z + "spline", (P, Q, zm(N=2, in_=(0x3fffffff, 2)), P, P, None)),
        "zoom2d_spline/out_cells_over": (z + "spline", (P, Q, zm(out=(65536, 32768)), P, P, None)),
        "zoom2d_spline/same_buffer": (z + "spline", (P, P, zm(), P, P, None)),
        "zoom2d_spline/taps_3": (z + "spline", (P, Q, zm(taps=3), P, P, None)),
        "zoom2d_spline/f64_two_taps": (z + "spline", (P, Q, zm(in_dtype=L.DLKA_F64), P, P, None)),
        "zoom2d_spline/f32_four_taps": (z + "spline", (P, Q, zm(taps=4), P, P, None)),
        "zoom2d_spline/bf16_to_f32": (z + "spline", (P, Q, zm(in_dtype=L.DLKA_BF16), P, P, None)),
        "zoom2d_spline/out_dtype_7": (z + "spline", (P, Q, zm(out_dtype=7), P, P, None)),
        "zoom2d_spline/four_taps_out_f64": (z + "spline", (P, Q, zm(taps=4, in_dtype=L.DLKA_F64, out_dtype=L.DLKA_F64), P, P, None)),
        "zoom2d_spline/normalize_int16": (z + "spline", (P, Q, zm(in_dtype=3, out_dtype=3, normalize=1), P, P, None)),
        "zoom2d_spline/normalize_std_zero": (z + "spline", (P, Q, zm(normalize=1, std=0.), P, P, None)),
        "zoom2d_spline/in0_over+out1_zero": (z + "spline", (P, Q, zm(in_=(0x40000000, 1), out=(4, 0)), P, P, None)),
        "zoom2d_spline/in1_over+out0_zero": (z + "spline", (P, Q, zm(in_=(1, 0x40000000), out=(0, 4)), P, P, None)),
        "zoom2d_spline/N_over+in0_zero": (z + "spline", (P, Q, zm(N=2 ** 31, in_=(0, 4)), P, P, None)),
        "zoom2d_spline/N_over+in1_zero": (z + "spline", (P, Q, zm(N=2 ** 31, in_=(4, 0)), P, P, None)),
        "zoom2d_spline/null_src+dtype": (z + "spline", (None, Q, zm(out_dtype=7), P, P, None)),
        "zoom2d_spline/same_buffer+dtype": (z + "spline", (P, P, zm(out_dtype=7), P, P, None)),
        "zoom2d_spline/taps_3+dtype": (z + "spline", (P, Q, zm(taps=3, out_dtype=7), P, P, None)),
        "zoom2d_nearest/null_idx": (z + "nearest", (P, Q, zm(), 4, None, None)),
        "zoom2d_nearest/bytes_3": (z + "nearest", (P, Q, zm(), 3, P, None)),
        "zoom2d_nearest/bytes_16": (z + "nearest", (P, Q, zm(), 16, P, None)),
        "zoom2d_nearest/same_buffer": (z + "nearest", (P, P, zm(), 4, P, None)),
        "zoom2d_nearest/same_buffer+bytes": (z + "nearest", (P, P, zm(), 3, P, None)),
        "zoom2d_nearest/out_zero": (z + "nearest", (P, Q, zm(out=(0, 4)), 4, P, None)),
        "zoom2d_nearest/out_zero+null_x": (z + "nearest", (None, Q, zm(out=(0, 4)), 4, P, None)),
        "zoom2d_argmax/null_desc": (z + "argmax", (P, Q, None, 2, P, None)),
        "zoom2d_argmax/K_zero": (z + "argmax", (P, Q, zm(), 0, P, None)),
        "zoom2d_argmax/K_over": (z + "argmax", (P, Q, zm(), L.DLKA_ZOOM2D_K_MAX + 1, P, None)),
        "zoom2d_argmax/f64": (z + "argmax", (P, Q, zm(in_dtype=L.DLKA_F64), 2, P, None)),
        "zoom2d_argmax/int16": (z + "argmax", (P, Q, zm(in_dtype=3), 2, P, None)),
        "zoom2d_argmax/K_zero+dtype": (z + "argmax", (P, Q, zm(in_dtype=L.DLKA_F64), 0, P, None)),
        "zoom2d_argmax/K_over+dtype": (z + "argmax", (P, Q, zm(in_dtype=L.DLKA_F64), 256, P, None)),
        # ---- cl_resample ----
        "resample_argmax/null_desc": (r + "argmax", (P, Q, None, P, P, None, None)),
        "resample_argmax/C_zero": (r + "argmax", (P, Q, rs(C=0), P, P, None, None)),
        "resample_argmax/in_zero": (r + "argmax", (P, Q, rs(in_=(3, 0, 5)), P, P, None, None)),
        "resample_argmax/in_over": (r + "argmax", (P, Q, rs(in_=(2 ** 31, 1, 1)), P, P, None, None)),
        "resample_argmax/out_over": (r + "argmax", (P, Q, rs(out=(1, 1, 2 ** 31)), P, P, None, None)),
        "resample_argmax/in_cells_over": (r + "argmax", (P, Q, rs(in_=BIG3), P, P, None, None)),
        "resample_argmax/out_cells_over": (r + "argmax", (P, Q, rs(out=BIG3), P, P, None, None)),
        "resample_argmax/taps_3": (r + "argmax", (P, Q, rs(taps=(3, 2, 2)), P, P, None, None)),
        "resample_argmax/taps_4": (r + "argmax", (P, Q, rs(taps=(1, 2, 4)), P, P, None, None)),
        "resample_argmax/bf16": (r + "argmax", (P, Q, rs(dtype=L.DLKA_BF16), P, P, None, None)),
        "resample_argmax/C_257": (r + "argmax", (P, Q, rs(C=257), P, P, None, None)),
        "resample_argmax/taps0+in1_zero": (r + "argmax", (P, Q, rs(taps=(3, 2, 2), in_=(3, 0, 5)), P, P, None, None)),
        "resample_argmax/taps1+in0_zero": (r + "argmax", (P, Q, rs(taps=(1, 3, 2), in_=(0, 4, 5)), P, P, None, None)),
        "resample_argmax/in_cells_over+out2_zero": (r + "argmax", (P, Q, rs(in_=BIG3, out=(4, 5, 0)), P, P, None, None)),
        "resample_argmax/null_x+dtype": (r + "argmax", (None, Q, rs(dtype=L.DLKA_BF16), P, P, None, None)),
        "resample_argmax/dtype+C_257": (r + "argmax", (P, Q, rs(dtype=L.DLKA_BF16, C=257), P, P, None, None)),
        "resample_linear/null_w": (r + "linear", (P, Q, rs(), P, None, None)),
        "resample_linear/same_buffer": (r + "linear", (P, P, rs(), P, P, None)),
        "resample_linear/dtype_3": (r + "linear", (P, Q, rs(dtype=3), P, P, None)),
        "resample_linear/same_buffer+dtype": (r + "linear", (P, P, rs(dtype=3), P, P, None)),
        "resample_labels/same_buffer": (r + "labels", (P, P, rs(), P, P, 0, None)),
        "resample_labels/out_zero": (r + "labels", (P, Q, rs(out=(0, 5, 6)), P, P, 0, None)),
        "resample_labels/channels_cells_over": (r + "labels", (P, Q, rs(C=3, out=(65536, 16384, 1)), P, P, 0, None)),
        "resample_spline_eval/two_taps": (r + "spline_eval", (P, Q, rs(), P, P, P, P, -1, None)),
        "resample_spline_eval/clip_axis_3": (r + "spline_eval", (P, Q, rs(taps=(4, 4, 4)), P, P, P, P, 3, None)),
        "resample_spline_eval/C_2": (r + "spline_eval", (P, Q, rs(taps=(4, 4, 4), C=2), P, P, P, P, -1, None)),
        "resample_spline_eval/clip_axis+C_2": (r + "spline_eval", (P, Q, rs(taps=(4, 4, 4), C=2), P, P, P, P, 3, None)),
        "resample_spline_eval/null_lo": (r + "spline_eval", (P, Q, rs(taps=(4, 1, 4)), P, P, None, P, -1, None)),
        # ---- cl_spline ----
        "spline_pad/null_in": _pad(n=None),
        "spline_pad/bf16": _pad(dtype=L.DLKA_BF16),
        "spline_pad/int16": _pad(dtype=3),
        "spline_pad/dtype+in_zero": _pad(dtype=L.DLKA_BF16, n=(0, 4, 5)),
        "spline_pad/in_zero": _pad(n=(3, 0, 5)),
        "spline_pad/pad_negative": _pad(pad=(1, -1, 1)),
        "spline_pad/pad_65": _pad(pad=(1, 1, 65)),
        "spline_pad/in_over": _pad(n=(LIM - 127, 1, 1), pad=(0, 0, 0)),
        "spline_pad/cells_over": _pad(n=BIG3),
        "spline_pad/padded_cells_over": _pad(n=(46340, 46340, 1), pad=(1, 1, 0)),
        "spline_pad/in0_over+pad1_negative": _pad(n=(LIM - 127, 1, 1), pad=(0, -1, 0)),
        "spline_pad/pad0_negative+in0_over": _pad(n=(LIM - 127, 1, 1), pad=(-1, 0, 0)),
        "spline_pad/pad0_65+in1_zero": _pad(n=(3, 0, 5), pad=(65, 0, 0)),
        "spline_prefilter/null_ext": _pre(ext=None),
        "spline_prefilter/axis_3": _pre(axis=3),
        "spline_prefilter/boundary_9": _pre(boundary=9),
        "spline_prefilter/ext_zero": _pre(ext=(3, 4, 0)),
        "spline_prefilter/ext_over": _pre(ext=(2 ** 31, 1, 1)),
        "spline_prefilter/cells_over": _pre(ext=BIG3),
        "spline_prefilter/axis+boundary": _pre(axis=-1, boundary=9),
        "spline_prefilter/boundary+ext_zero": _pre(boundary=9, ext=(0, 4, 5)),
        "spline_prefilter/ext0_over+ext1_zero": _pre(ext=(2 ** 31, 0, 1)),
        # ---- cl_augment ----
        "augment_spatial/null_desc": (a + "spatial", (P, None, Q, None, P, P, None)),
        "augment_spatial/B_zero": (a + "spatial", (P, None, Q, ag(B=0), P, P, None)),
        "augment_spatial/pad_negative": (a + "spatial", (P, None, Q, ag(pad=-1), P, P, None)),
        "augment_spatial/mode_7": (a + "spatial", (P, None, Q, ag(mode=7), P, P, None)),
        "augment_spatial/pad_65": (a + "spatial", (P, P, Q, ag(pad=65, order=3), P, P, None)),
        "augment_spatial/pad_negative+mode": (a + "spatial", (P, None, Q, ag(pad=-1, mode=7), P, P, None)),
        "augment_spatial/src_zero": (a + "spatial", (P, None, Q, ag(src=(3, 0, 5)), P, P, None)),
        "augment_spatial/src_over": (a + "spatial", (P, None, Q, ag(src=(over_aug, 1, 1)), P, P, None)),
        "augment_spatial/out_over": (a + "spatial", (P, None, Q, ag(out=(2 ** 31, 1, 1)), P, P, None)),
        "augment_spatial/src_cells_over": (a + "spatial", (P, None, Q, ag(src=BIG3), P, P, None)),
        "augment_spatial/padded_cells_over": (a + "spatial", (P, P, Q, ag(src=(46340, 46340, 1), pad=1, order=3), P, P, None)),
        "augment_spatial/out_cells_over": (a + "spatial", (P, None, Q, ag(out=BIG3), P, P, None)),
        "augment_spatial/src0_over+out0_zero": (a + "spatial", (P, None, Q, ag(src=(over_aug, 1, 1), out=(0, 4, 6)), P, P, None)),
        "augment_spatial/src1_over+out0_zero": (a + "spatial", (P, None, Q, ag(src=(1, over_aug, 1), out=(0, 4, 6)), P, P, None)),
        "augment_spatial/src0_over+out1_zero": (a + "spatial", (P, None, Q, ag(src=(over_aug, 1, 1), out=(3, 0, 6)), P, P, None)),
        "augment_spatial/lanes_over": (a + "spatial", (P, None, Q, ag(B=32768, C=32768, out=(1024, 1024, 1024)), P, P, None)),
        "augment_spatial/null_x": (a + "spatial", (None, None, Q, ag(), P, P, None)),
        "augment_spatial/same_buffer": (a + "spatial", (P, None, P, ag(), P, P, None)),
        "augment_spatial/order_2": (a + "spatial", (P, None, Q, ag(order=2), P, P, None)),
        "augment_spatial/order_3_no_coef": (a + "spatial", (P, None, Q, ag(order=3, pad=2), P, P, None)),
        "augment_spatial/order_1_pad": (a + "spatial", (P, None, Q, ag(pad=2), P, P, None)),
        "augment_spatial/dtype_4": (a + "spatial", (P, None, Q, ag(dtype=4), P, P, None)),
        "augment_spatial/dtype_negative": (a + "spatial", (P, None, Q, ag(dtype=-1), P, P, None)),
        "augment_spatial/order_2+dtype": (a + "spatial", (P, None, Q, ag(order=2, dtype=4), P, P, None)),
        "augment_spatial/src_zero+null_x": (a + "spatial", (None, None, Q, ag(src=(0, 4, 5)), P, P, None)),
        "augment_spatial2d/third_extent": (a + "spatial2d", (P, None, Q, ag2(src=(4, 5, 1)), P, P, None)),
        "augment_spatial2d/src_zero": (a + "spatial2d", (P, None, Q, ag2(src=(0, 5, 0)), P, P, None)),
        "augment_spatial2d/src_over": (a + "spatial2d", (P, None, Q, ag2(src=(4, over_aug, 0)), P, P, None)),
        "augment_spatial2d/dtype_4": (a + "spatial2d", (P, None, Q, ag2(dtype=4), P, P, None)),
        "augment_spatial2d/third_extent+mode": (a + "spatial2d", (P, None, Q, ag2(out=(4, 6, 2), mode=7), P, P, None)),
        "augment_spatial_labels/same_buffer": (a + "spatial_labels", (P, P, ag(), P, P, None)),
        "augment_spatial_labels/pad_1": (a + "spatial_labels", (P, Q, ag(pad=1), P, P, None)),
        "augment_spatial_labels/order_3": (a + "spatial_labels", (P, Q, ag(order=3), P, P, None)),
        "augment_spatial_labels/cval_0.7": (a + "spatial_labels", (P, Q, ag(cval=0.7), P, P, None)),
        "augment_spatial_labels/order_0_cval_1e10": (a + "spatial_labels", (P, Q, ag(order=0, cval=1e10), P, P, None)),
        "augment_spatial_labels/null_maps": (a + "spatial_labels", (P, Q, ag(), None, P, None)),
        "augment_spatial_labels/out_zero+null_seg": (a + "spatial_labels", (None, Q, ag(out=(3, 4, 0)), P, P, None)),
        "augment_spatial2d_labels/order_3": (a + "spatial2d_labels", (P, Q, ag2(order=3), P, P, None)),
        "augment_spatial2d_labels/third_extent": (a + "spatial2d_labels", (P, Q, ag2(out=(4, 6, 1)), P, P, None)),
        "augment_gaussian/null_ext": _gauss(ext=None),
        "augment_gaussian/null_radius": _gauss(radius=None),
        "augment_gaussian/same_buffer": _gauss(y=P),
        "augment_gaussian/axis_3": _gauss(axis=3),
        "augment_gaussian/channels_zero": _gauss(ch=0),
        "augment_gaussian/dtype_4": _gauss(dtype=4),
        "augment_gaussian/dtype_negative": _gauss(dtype=-1),
        "augment_gaussian/ext_zero": _gauss(ext=(3, 0, 5)),
        "augment_gaussian/ext_over": _gauss(ext=(0x40000000, 1, 1)),
        "augment_gaussian/cells_over": _gauss(ext=BIG3),
        "augment_gaussian/channels_over": _gauss(ch=2 ** 31),
        "augment_gaussian/total_over": _gauss(ch=LIM, ext=(1024, 1, 1)),
        "augment_gaussian/same_buffer+axis": _gauss(y=P, axis=3),
        "augment_gaussian/axis+dtype": _gauss(axis=3, dtype=4),
        "augment_gaussian/dtype+ext_zero": _gauss(dtype=4, ext=(0, 4, 5)),
        "augment_gaussian/ext0_over+ext1_zero": _gauss(ext=(0x40000000, 0, 1)),
        "augment_channel_stats/null_x": _stats(x=None),
        "augment_channel_stats/channels_zero": _stats(ch=0),
        "augment_channel_stats/channels_65536": _stats(ch=65536),
        "augment_channel_stats/cells_over": _stats(cells=2 ** 31),
        "augment_channel_stats/dtype_4": _stats(dtype=4),
        "augment_channel_stats/null_workspace": _stats(ws=None),
        "augment_channel_stats/small_workspace": _stats(nbytes=8),
        "augment_channel_stats/misaligned_workspace": _stats(ws=Q + 4),
        "augment_channel_stats/dtype+null_workspace": _stats(dtype=4, ws=None),
        "augment_channel_stats/cells_over+dtype": _stats(cells=2 ** 31, dtype=4),
        "augment_pointwise/null_ops": _point(ops=None),
        "augment_pointwise/same_buffer": _point(y=P),
        "augment_pointwise/B_zero": _point(B=0),
        "augment_pointwise/dtype_4": _point(dtype=4),
        "augment_pointwise/ext_zero": _point(ext=(3, 4, 0)),
        "augment_pointwise/ext_over": _point(ext=(2 ** 31, 1, 1)),
        "augment_pointwise/cells_over": _point(ext=BIG3),
        "augment_pointwise/channels_over": _point(B=65536, C=65536),
        "augment_pointwise/blocks_over": _point(B=46340, C=46340, ext=(1024, 1024, 1024)),
        "augment_pointwise/B_zero+dtype": _point(B=0, dtype=4),
        "augment_pointwise/dtype+ext_zero": _point(dtype=4, ext=(0, 4, 5)),
        "augment_pointwise/ext_zero+channels_over": _point(ext=(3, 4, 0), B=65536, C=65536),
        # ---- cl_preprocess ----
        "prep_background/null_desc": (t + "background", (P, None, Q, None)),
        "prep_background/rank_1": (t + "background", (P, pp(rank=1), Q, None)),
        "prep_background/C_zero": (t + "background", (P, pp(C=0), Q, None)),
        "prep_background/C_over": (t + "background", (P, pp(C=L.DLKA_PREP_C_MAX + 1), Q, None)),
        "prep_background/ext_zero": (t + "background", (P, pp(ext=(3, 0, 5)), Q, None)),
        "prep_background/ext_over": (t + "background", (P, pp(ext=(1, 2 ** 31, 1)), Q, None)),
        "prep_background/cells_over": (t + "background", (P, pp(ext=BIG3), Q, None)),
        "prep_background/rank_2_depth_2": (t + "background", (P, pp(rank=2, ext=(2, 4, 5)), Q, None)),
        "prep_background/rank_2_depth_2+cells_over": (t + "background", (P, pp(rank=2, ext=(2, 65536, 65536)), Q, None)),
        "prep_background/C_over+ext_zero": (t + "background", (P, pp(C=33, ext=(0, 4, 5)), Q, None)),
        "prep_background/null_data": (t + "background", (None, pp(), Q, None)),
        "prep_fill_bbox/null_labels": (t + "fill_bbox", (P, None, pp(), Q, 256, Q, Q, None)),
        "prep_fill_bbox/null_workspace": (t + "fill_bbox", (P, P, pp(), None, 256, Q, Q, None)),
        "prep_fill_bbox/small_workspace": (t + "fill_bbox", (P, P, pp(), Q, 60, Q, Q, None)),
        "prep_mask_bbox/null_box": (t + "mask_bbox", (P, pp(), None, None)),
        "prep_mask_bbox/ext_zero": (t + "mask_bbox", (P, pp(ext=(3, 4, 0)), Q, None)),
        "prep_crop/seg_channels_negative": (t + "crop", (P, None, None, pp(seg_channels=-1), Q, None, None)),
        "prep_crop/seg_channels_over": (t + "crop", (P, None, None, pp(seg_channels=33), Q, None, None)),
        "prep_crop/lo_negative": (t + "crop", (P, None, None, pp(lo=(-1, 0, 0)), Q, None, None)),
        "prep_crop/empty_box": (t + "crop", (P, None, None, pp(lo=(0, 2, 0), hi=(3, 2, 5)), Q, None, None)),
        "prep_crop/box_beyond": (t + "crop", (P, None, None, pp(hi=(3, 4, 6)), Q, None, None)),
        "prep_crop/same_buffer": (t + "crop", (P, None, None, pp(), P, None, None)),
        "prep_crop/seg_out_without_mask": (t + "crop", (P, None, None, pp(), Q, Q, None)),
        "prep_crop/seg_out_without_seg": (t + "crop", (P, None, P, pp(seg_channels=1), Q, Q, None)),
        "prep_crop/ext_zero+box": (t + "crop", (P, None, None, pp(ext=(0, 4, 5), lo=(-1, 0, 0)), Q, None, None)),
        "prep_channel_stats/null_seg": (t + "channel_stats", (P, None, pp(), Q, Q, 256, None)),
        "prep_channel_stats/null_workspace": (t + "channel_stats", (P, P, pp(), Q, None, 256, None)),
        "prep_channel_stats/misaligned_workspace": (t + "channel_stats", (P, P, pp(), Q, Q + 4, 200, None)),
        "prep_normalize/null_table": (t + "normalize", (P, P, pp(), None, Q, None)),
        "prep_normalize/rank_4": (t + "normalize", (P, P, pp(rank=4), P, Q, None)),
        # ---- cl_surface_dist ----
        "sd_label_stats/null_desc": ("dlka_sd_label_stats", (P, P, None, Q, 256, Q, None)),
        "sd_label_stats/rank_4": ("dlka_sd_label_stats", (P, P, sd(rank=4), Q, 256, Q, None)),
        "sd_label_stats/connectivity_zero": ("dlka_sd_label_stats", (P, P, sd(connectivity=0), Q, 256, Q, None)),
        "sd_label_stats/connectivity_over_rank": ("dlka_sd_label_stats", (P, P, sd(rank=2, connectivity=3, ext=(1, 4, 5)), Q, 256, Q, None)),
        "sd_label_stats/label_dtype_4": ("dlka_sd_label_stats", (P, P, sd(label_dtype=4), Q, 256, Q, None)),
        "sd_label_stats/label_dtype_negative": ("dlka_sd_label_stats", (P, P, sd(label_dtype=-1), Q, 256, Q, None)),
        "sd_label_stats/K_zero": ("dlka_sd_label_stats", (P, P, sd(K=0), Q, 256, Q, None)),
        "sd_label_stats/K_over": ("dlka_sd_label_stats", (P, P, sd(K=L.DLKA_SD_K_MAX + 1), Q, 256, Q, None)),
        "sd_label_stats/ext_zero": ("dlka_sd_label_stats", (P, P, sd(ext=(3, 0, 5)), Q, 256, Q, None)),
        "sd_label_stats/ext_over": ("dlka_sd_label_stats", (P, P, sd(ext=(2 ** 31, 1, 1)), Q, 256, Q, None)),
        "sd_label_stats/cells_over": ("dlka_sd_label_stats", (P, P, sd(ext=(65536, 65536, 1)), Q, 256, Q, None)),
        "sd_label_stats/rank_2_depth_2": ("dlka_sd_label_stats", (P, P, sd(rank=2, ext=(2, 4, 5)), Q, 256, Q, None)),
        "sd_label_stats/line_over": ("dlka_sd_label_stats", (P, P, sd(ext=(1, 1, 32769)), Q, 256, Q, None)),
        "sd_label_stats/spacing_zero": ("dlka_sd_label_stats", (P, P, sd(spacing=(1., 0., 1.)), Q, 256, Q, None)),
        "sd_label_stats/spacing_nan": ("dlka_sd_label_stats", (P, P, sd(spacing=(float("nan"), 1., 1.)), Q, 256, Q, None)),
        "sd_label_stats/label_dtype+K_zero": ("dlka_sd_label_stats", (P, P, sd(label_dtype=4, K=0), Q, 256, Q, None)),
        "sd_label_stats/connectivity+label_dtype": ("dlka_sd_label_stats", (P, P, sd(connectivity=0, label_dtype=4), Q, 256, Q, None)),
        "sd_label_stats/cells_over+ext2_over": ("dlka_sd_label_stats", (P, P, sd(ext=(65536, 65536, 2 ** 31)), Q, 256, Q, None)),
        "sd_label_stats/line_over+spacing": ("dlka_sd_label_stats", (P, P, sd(ext=(1, 1, 32769), spacing=(1., 1., 0.)), Q, 256, Q, None)),
        "sd_label_stats/null_prediction": ("dlka_sd_label_stats", (None, P, sd(), Q, 256, Q, None)),
        "sd_label_stats/null_workspace": ("dlka_sd_label_stats", (P, P, sd(), None, 256, Q, None)),
        "sd_label_stats/small_workspace": ("dlka_sd_label_stats", (P, P, sd(), Q, 16, Q, None)),
        "sd_distances/null_boxes": ("dlka_sd_distances", (P, P, sd(), None, Q, 4096, Q, 4096, None)),
        "sd_distances/box_negative": ("dlka_sd_distances", (P, P, sd(), BOX(-1, 0, 0, 3, 4, 5), Q, 4096, Q, 4096, None)),
        "sd_distances/box_beyond": ("dlka_sd_distances", (P, P, sd(), BOX(1, 0, 0, 3, 4, 5), Q, 4096, Q, 4096, None)),
        "sd_distances/null_sqdist": ("dlka_sd_distances", (P, P, sd(), BOX(0, 0, 0, 3, 4, 5), Q, 4096, None, 4096, None)),
        "sd_distances/small_sqdist": ("dlka_sd_distances", (P, P, sd(), BOX(0, 0, 0, 3, 4, 5), Q, 4096, Q, 1, None)),
        "sd_distances/null_workspace": ("dlka_sd_distances", (P, P, sd(), BOX(0, 0, 0, 3, 4, 5), None, 4096, Q, 4096, None)),
        "sd_distances/small_workspace": ("dlka_sd_distances", (P, P, sd(), BOX(0, 0, 0, 3, 4, 5), Q, 100, Q, 4096, None)),
        "sd_distances/empty_boxes": ("dlka_sd_distances", (P, P, sd(), BOX(0, 0, 0, 0, 4, 5), None, 0, None, 0, None)),
        "sd_distances/label_dtype_4": ("dlka_sd_distances", (P, P, sd(label_dtype=4), BOX(0, 0, 0, 3, 4, 5), Q, 4096, Q, 4096, None)),
        # ---- cl_conn_comp ----
        "cc_components/null_desc": ("dlka_cc_components", (P, None, Q, 4096, Q, None, Q, None)),
        "cc_components/rank_zero": ("dlka_cc_components", (P, cc(rank=0), Q, 4096, Q, None, Q, None)),
        "cc_components/connectivity_4": ("dlka_cc_components", (P, cc(connectivity=4), Q, 4096, Q, None, Q, None)),
        "cc_components/label_dtype_9": ("dlka_cc_components", (P, cc(label_dtype=9), Q, 4096, Q, None, Q, None)),
        "cc_components/label_dtype_negative": ("dlka_cc_components", (P, cc(label_dtype=-1), Q, 4096, Q, None, Q, None)),
        "cc_components/K_zero": ("dlka_cc_components", (P, cc(K=0), Q, 4096, Q, None, Q, None)),
        "cc_components/ext_zero": ("dlka_cc_components", (P, cc(ext=(3, 4, 0)), Q, 4096, Q, None, Q, None)),
        "cc_components/ext_over": ("dlka_cc_components", (P, cc(ext=(2 ** 31, 1, 1)), Q, 4096, Q, None, Q, None)),
        "cc_components/cells_over": ("dlka_cc_components", (P, cc(ext=BIG3), Q, 4096, Q, None, Q, None)),
        "cc_components/rank_2_depth_2": ("dlka_cc_components", (P, cc(rank=2, ext=(2, 4, 5)), Q, 4096, Q, None, Q, None)),
        "cc_components/rank_1_height_2": ("dlka_cc_components", (P, cc(rank=1, ext=(1, 2, 5)), Q, 4096, Q, None, Q, None)),
        "cc_components/mask_mode_K_2": ("dlka_cc_components", (P, cc(mask_mode=1, K=2), Q, 4096, Q, None, Q, None)),
        "cc_components/n_ids_zero": ("dlka_cc_components", (P, cc(n_ids=0), Q, 4096, Q, None, Q, None)),
        "cc_components/entry_of_5": ("dlka_cc_components", (P, cc(entry_of=(5,)), Q, 4096, Q, None, Q, None)),
        "cc_components/duplicate_ids": ("dlka_cc_components", (P, cc(n_ids=2, class_id=(1, 1), entry_of=(0, 0)), Q, 4096, Q, None, Q, None)),
        "cc_components/min_count_negative": ("dlka_cc_components", (P, cc(has_min=1, min_count=(-1,)), Q, 4096, Q, None, Q, None)),
        "cc_components/label_dtype+K_zero": ("dlka_cc_components", (P, cc(label_dtype=9, K=0), Q, 4096, Q, None, Q, None)),
        "cc_components/ext0_over+ext1_zero": ("dlka_cc_components", (P, cc(ext=(2 ** 31, 0, 1)), Q, 4096, Q, None, Q, None)),
        "cc_components/cells_over+rank_2_depth": ("dlka_cc_components", (P, cc(rank=2, ext=(65536, 65536, 1)), Q, 4096, Q, None, Q, None)),
        "cc_components/null_image": ("dlka_cc_components", (None, cc(), Q, 4096, Q, None, Q, None)),
        "cc_components/filtered_is_image": ("dlka_cc_components", (P, cc(), Q, 4096, Q, P, Q, None)),
        "cc_components/null_workspace": ("dlka_cc_components", (P, cc(), None, 4096, Q, None, Q, None)),
        "cc_components/small_workspace": ("dlka_cc_components", (P, cc(), Q, 100, Q, None, Q, None)),
        "cc_component_table/capacity_negative": ("dlka_cc_component_table", (cc(), Q, 4096, -1, Q, Q, None)),
        "cc_component_table/capacity_zero": ("dlka_cc_component_table", (cc(), Q, 4096, 0, Q, Q, None)),
        "cc_component_table/null_sizes": ("dlka_cc_component_table", (cc(), Q, 4096, 1, None, Q, None)),
        "cc_component_table/null_workspace": ("dlka_cc_component_table", (cc(), None, 4096, 1, Q, Q, None)),
        "cc_component_table/label_dtype_9": ("dlka_cc_component_table", (cc(label_dtype=9), Q, 4096, 1, Q, Q, None)),
        # ---- cl_tiles ----
        "tiles_gather/null_x": _gather(x=None),
        "tiles_gather/C_zero": _gather(C=0),
        "tiles_gather/pad_negative": _gather(pad=(0, -1, 0)),
        "tiles_gather/null_origins": _gather(org=None),
        "tiles_gather/T_zero": _gather(T=0),
        "tiles_gather/T_over": _gather(T=L.DLKA_TILES_MAX_T + 1),
        "tiles_gather/M_9": _gather(M=9),
        "tiles_gather/mask_8": _gather(msk=ci(8)),
        "tiles_gather/blocks_over": _gather(C=LIM, p=(32768, 32768, 2)),
        "tiles_gather/C_zero+null_origins": _gather(C=0, org=None),
        "tiles_gather/T_zero+M_9": _gather(T=0, M=9),
        "tiles_blend/null_logits": _blend(x=None),
        "tiles_blend/f64": _blend(dtype=L.DLKA_F64),
        "tiles_blend/dtype_3": _blend(dtype=3),
        "tiles_blend/K_zero": _blend(K=0),
        "tiles_blend/K_over": _blend(K=L.DLKA_TILES_K_MAX + 1),
        "tiles_blend/nonlin_9": _blend(nl=9),
        "tiles_blend/dtype+K_zero": _blend(dtype=L.DLKA_F64, K=0),
        "tiles_blend/K_over+null_masks": _blend(K=33, msk=None),
        "tiles_blend/tile_outside": _blend(org=ci(3, 0, 0)),
        "tiles_blend/null_masks": _blend(msk=None),
        "tiles_finalize/null_score": _final(score=None),
        "tiles_finalize/K_zero": _final(K=0),
        "tiles_finalize/kept_beyond": _final(pad=(1, 0, 0)),
        # ---- cl_seg_loss ----
        "seg_loss_forward/null_desc": ("dlka_seg_loss_forward", (P, P, None, Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/B_zero": ("dlka_seg_loss_forward", (P, P, sl(B=0), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/B_65536": ("dlka_seg_loss_forward", (P, P, sl(B=65536), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/f64": ("dlka_seg_loss_forward", (P, P, sl(dtype=L.DLKA_F64), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/label_dtype_2": ("dlka_seg_loss_forward", (P, P, sl(label_dtype=2), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/K_over": ("dlka_seg_loss_forward", (P, P, sl(K=L.DLKA_SEG_LOSS_K_MAX + 1), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/mode_9": ("dlka_seg_loss_forward", (P, P, sl(mode=9), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/N_over": ("dlka_seg_loss_forward", (P, P, sl(N=2 ** 40), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/dtype+K_over": ("dlka_seg_loss_forward", (P, P, sl(dtype=L.DLKA_F64, K=33), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/B_zero+dtype": ("dlka_seg_loss_forward", (P, P, sl(B=0, dtype=L.DLKA_F64), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/null_logits": ("dlka_seg_loss_forward", (None, P, sl(), Q, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/null_workspace": ("dlka_seg_loss_forward", (P, P, sl(), None, 4096, Q, Q, Q, Q, None)),
        "seg_loss_forward/small_workspace": ("dlka_seg_loss_forward", (P, P, sl(), Q, 8, Q, Q, Q, Q, None)),
        "seg_loss_backward/null_coef": ("dlka_seg_loss_backward", (P, P, sl(), None, P, Q, None)),
        "seg_loss_backward/label_dtype_2": ("dlka_seg_loss_backward", (P, P, sl(label_dtype=2), P, P, Q, None)),
        "seg_eval_counts/K_1": ("dlka_seg_eval_counts", (P, P, sl(K=1), Q, 4096, Q, None)),
        "seg_eval_counts/K_1+null_workspace": ("dlka_seg_eval_counts", (P, P, sl(K=1), None, 4096, Q, None)),
        "seg_eval_counts/null_counts+K_1": ("dlka_seg_eval_counts", (P, P, sl(K=1), Q, 4096, None, None)),
    }
    return c


def run(lib):
    """{id: status} over cases(); lib: a library bound by deformablelka_amd._lib.bind."""
    out = {}
    for cid, (name, args) in cases().items():
        out[cid] = int(getattr(lib, name)(*args))
    return out
