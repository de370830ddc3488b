"""Drop-in for `models.hovernet.post_proc.process`
(/root/reference/models/hovernet/post_proc.py:94-186) on the GPU.

* `process(pred_map, nr_types=None, return_centroids=False)` keeps the reference's
  signature and return contract `(pred_inst int32 [H,W], inst_info_dict | None)` for one
  host map; it is a thin wrapper over the batched device path.
* `process_batch_device(pred_dev, nr_types)` is the north-star path: `[N,h,w,3|4]` float32
  maps already in HBM (straight from `run_desc.infer_step_device`) -> int32 instance maps
  and the per-instance table in HBM, no CPU round trip per tile; `return_contours=True` adds the
  contours, traced in HBM too.

Instance separation (`__proc_np_hv`, post_proc.py:26-90) and the array half of the
per-instance loop (bbox / centroid / type vote, post_proc.py:119-181) are HIP kernels in
libhvn_hip.so.  Contour tracing (`cv2.findContours`, post_proc.py:132-135) has two forms in the same
library with bit-equal results: the host routine over each instance's bbox crop (csrc/hvn_contour.cpp,
any label map; the default everywhere) and, opt-in, a mark-free border walk on the device
(csrc/hvn_contour_dev.hip: `PostProc.contours`, `trace_contours_device`, `process(contours="device")`)
for maps in which every label is one 8-connected piece -- which the instance separation's output is.
No CPU fallback exists for the GPU stages.
"""
import ctypes

import numpy as np
import torch

from . import features as F
from . import lib as L
from . import texture as TX


def _check_image(image, nhw, device):
    """The RGB image that goes with `nhw` = (N, h, w) label maps on `device`: uint8 device tensor [N,h,w,3]."""
    if not torch.is_tensor(image) or image.dtype != torch.uint8:
        raise TypeError("image must be a uint8 tensor, got %s" % (image.dtype if torch.is_tensor(image) else type(image).__name__))
    if tuple(image.shape) != tuple(nhw) + (3,):
        raise ValueError("image %s does not match the maps: expected %s" % (tuple(image.shape), tuple(nhw) + (3,)))
    if image.device != device:
        raise ValueError("image is on %s, the maps on %s" % (image.device, device))


class PostProc:
    """Owns the device workspace for `n` maps of `h x w` (grown on demand)."""

    def __init__(self, device="cuda"):
        L.require_gpu()
        self.device = torch.device(device)
        self._ws = None
        self._tws = None
        self._cws = None
        self._cpin = None
        self._fws = None

    def _workspace(self, n, h, w):
        self._ws = L.grown(self._ws, L.lib().hvn_postproc_workspace_bytes(n, h, w), self.device)
        return self._ws

    def separate(self, pred, taps=False):
        """pred: float32 device tensor [N,h,w,3|4] -> int32 device tensor [N,h,w]
        (+ (blb, dist, marker) stage taps when taps=True)."""
        assert pred.dtype == torch.float32 and pred.dim() == 4 and pred.is_cuda
        pred = pred.contiguous()
        n, h, w, c = pred.shape
        if c not in (3, 4):
            raise ValueError("prediction map must have 3 ([p,h,v]) or 4 ([type,p,h,v]) channels, got %d" % c)
        ws = self._workspace(n, h, w)
        self._last_nhw = (n, h, w)
        inst = torch.empty((n, h, w), dtype=torch.int32, device=self.device)
        stream = L.stream_ptr(self.device)
        if not taps:
            L.call("hvn_postproc", pred.data_ptr(), n, h, w, c, c - 3, inst.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            return inst
        blb = torch.empty((n, h, w), dtype=torch.int32, device=self.device)
        dist = torch.empty((n, h, w), dtype=torch.float64, device=self.device)
        marker = torch.empty((n, h, w), dtype=torch.int32, device=self.device)
        L.call("hvn_postproc_taps", pred.data_ptr(), n, h, w, c, c - 3, inst.data_ptr(), blb.data_ptr(), dist.data_ptr(),
               marker.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return inst, blb, dist, marker

    def flood_stats(self, stream=None):
        """Which replay the marker-controlled watershed of the LAST `separate` call took, summed over its maps (hvn_postproc_stats):
        dict of component counts; `whole_tile_replays` are the exact one-lane whole-tile fallbacks."""
        if self._ws is None or getattr(self, "_last_nhw", None) is None:
            return None
        n, h, w = self._last_nhw
        out = (ctypes.c_longlong * 10)()
        L.call("hvn_postproc_stats", self._ws.data_ptr(), self._ws.numel(), n, h, w, out, L.stream_ptr(self.device, stream))
        keys = ("components", "small_window", "bitmap_window", "hbm_window", "to_heap_by_marker_tie", "to_heap_by_full_frontier",
                "component_heap_replays", "whole_tile_replays", "maps_flagged", "largest_component_box")
        return {k: int(v) for k, v in zip(keys, out)}

    def table(self, inst, pred, nr_types):
        """-> (records uint8 view [N,max_inst,sizeof(rec)], counts int32 [N]) on the device."""
        n, h, w = inst.shape
        max_inst = h * w // 13 + 1   # an opened marker component holds at least one 13-px element
        nt = int(nr_types or 0)
        self._tws = L.grown(self._tws, L.lib().hvn_instance_table_workspace_bytes(n, max_inst, nt), self.device)
        rec = torch.empty((n, max_inst, ctypes.sizeof(L.hvn_inst_rec)), dtype=torch.uint8, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        L.call("hvn_instance_table", inst.data_ptr(), pred.data_ptr() if nt else None, n, h, w, pred.shape[-1], nt,
               rec.data_ptr(), counts.data_ptr(), max_inst, self._tws.data_ptr(), self._tws.numel(), L.stream_ptr(self.device))
        return rec, counts

    def contours(self, inst, rec, max_pts=None):
        """contours[0] of every record, traced on the device (hvn_trace_contours_device) on the current stream, no host sync.
        inst: int32 device tensor [N,h,w]; rec: `table`'s records [N,max_inst,sizeof(rec)].  PRECONDITION: every label of `inst`
        is one 8-connected piece (true of `separate`'s output); other maps go to `trace_contours_flat`.
        -> (pts int32 [max_pts,2] of (x, y), offs int64 [N*max_inst+1], status int32 [4]) on the device: the record at
        (map i, slot j) owns pts[offs[i*max_inst+j]:offs[i*max_inst+j+1]]; status = (flagged records -- they own no points --,
        1 if offs[-1] > max_pts: the records beyond max_pts were not written, smallest flagged i*max_inst+j or -1, 0).
        max_pts defaults to N*h*w // 4 (2 bytes per pixel; dense noise blobs need 0.14 points per pixel)."""
        assert inst.dtype == torch.int32 and inst.dim() == 3 and inst.is_cuda and rec.dtype == torch.uint8 and rec.dim() == 3 and rec.is_cuda
        inst, rec = inst.contiguous(), rec.contiguous()
        n, h, w = inst.shape
        max_inst = rec.shape[1]
        if rec.shape[0] != n or rec.shape[2] != ctypes.sizeof(L.hvn_inst_rec):
            raise ValueError("record table %s does not belong to %d maps" % (tuple(rec.shape), n))
        if max_pts is None:
            max_pts = n * h * w // 4
        max_pts = max(int(max_pts), 0)
        self._cws = L.grown(self._cws, L.lib().hvn_contours_workspace_bytes(n, max_inst), self.device)
        pts = torch.empty((max_pts, 2), dtype=torch.int32, device=self.device)
        offs = torch.empty((n * max_inst + 1,), dtype=torch.int64, device=self.device)
        status = torch.empty((4,), dtype=torch.int32, device=self.device)
        L.call("hvn_trace_contours_device", inst.data_ptr(), n, h, w, rec.data_ptr(), max_inst, pts.data_ptr() if max_pts else None,
               max_pts, offs.data_ptr(), status.data_ptr(), self._cws.data_ptr(), self._cws.numel(), L.stream_ptr(self.device))
        return pts, offs, status

    def features(self, inst, rec, image=None):
        """The morphometric sums of every record (hvn_instance_features) on the current stream, no host sync.
        inst: int32 device tensor [N,h,w]; rec: `table`'s records [N,max_inst,sizeof(rec)]; image: uint8 device tensor [N,h,w,3]
        (RGB; adds the colour sums) or None.  -> uint8 device tensor [N,max_inst,sizeof(hvn_inst_feat)]: `features.FEAT_DTYPE`
        slots parallel to the records; `features.derive` makes the float features of them on the host.  Any label map is valid;
        a table that was not made from `inst` shows as seen != area."""
        if not (torch.is_tensor(inst) and inst.dtype == torch.int32 and inst.dim() == 3 and inst.is_cuda):
            raise ValueError("inst must be an int32 device tensor [N,h,w]")
        n, h, w = inst.shape
        if not (torch.is_tensor(rec) and rec.dtype == torch.uint8 and rec.dim() == 3 and rec.is_cuda and rec.shape[0] == n
                and rec.shape[2] == ctypes.sizeof(L.hvn_inst_rec)):
            raise ValueError("record table does not belong to %d maps" % n)
        if image is not None:
            _check_image(image, (n, h, w), inst.device)
            image = image.contiguous()
        inst, rec = inst.contiguous(), rec.contiguous()
        max_inst = rec.shape[1]
        need = L.lib().hvn_instance_features_workspace_bytes(n, h, w, max_inst)
        if need:
            self._fws = L.grown(self._fws, need, self.device)
        feat = torch.empty((n, max_inst, ctypes.sizeof(L.hvn_inst_feat)), dtype=torch.uint8, device=self.device)
        L.call("hvn_instance_features", inst.data_ptr(), image.data_ptr() if image is not None else None, n, h, w, rec.data_ptr(),
               max_inst, feat.data_ptr(), self._fws.data_ptr() if need else None, need, L.stream_ptr(self.device))
        return feat

    def texture(self, inst, rec, image, scale="range", form=0):
        """The grey-level co-occurrence counts of every record (HVN_OP_INST_TEXTURE, hover_net_amd/texture.py) on the current
        stream, no host sync.  inst: int32 device tensor [N,h,w]; rec: `table`'s records [N,max_inst,sizeof(rec)]; image: uint8
        device tensor [N,h,w,3] (RGB), mandatory; scale: "range" (levels over the nucleus's own grey range) or "fixed" (over
        0..255).  -> uint8 device tensor [N,max_inst,1104]: `texture.TEX_DTYPE` slots parallel to the records, every byte written;
        `texture.derive` makes the float features of them on the host.  Any label map is valid; a table that was not made from
        `inst` shows as seen != area.  form: 0 = the product's kernel form (one LDS add per pair), 1 = the one that lost (equal keys
        merged first; tools/texture_bench.py)."""
        from . import plan as PL

        mode = TX.SCALES[TX.check_scale(scale)]
        if not (torch.is_tensor(inst) and inst.dtype == torch.int32 and inst.dim() == 3 and inst.is_cuda):
            raise ValueError("inst must be an int32 device tensor [N,h,w]")
        n, h, w = inst.shape
        if not (torch.is_tensor(rec) and rec.dtype == torch.uint8 and rec.dim() == 3 and rec.is_cuda and rec.shape[0] == n
                and rec.shape[2] == ctypes.sizeof(L.hvn_inst_rec)):
            raise ValueError("record table does not belong to %d maps" % n)
        if image is None:
            raise ValueError("texture needs the image")
        _check_image(image, (n, h, w), inst.device)
        inst, rec, image = inst.contiguous(), rec.contiguous(), image.contiguous()
        max_inst = rec.shape[1]
        tex = torch.empty((n, max_inst, TX.TEX_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        op = L.hvn_op()
        op.kind, op.cout, op._rsv, op.stride = PL.OP_INST_TEXTURE, max_inst, mode, int(form)
        op.x.base, op.x.h, op.x.w, op.x.c = image.data_ptr(), h, w, 3
        op.res.base, op.w, op.y.base = inst.data_ptr(), rec.data_ptr(), tex.data_ptr()
        L.call("hvn_run_op", ctypes.addressof(op), n, L.stream_ptr(self.device))
        return tex

    def _pinned(self, like):
        """Pinned host buffers for `contours`' three outputs (kept: pinned allocations are slow)."""
        if self._cpin is None or any(b.numel() < t.numel() for b, t in zip(self._cpin, like)):
            self._cpin = tuple(torch.empty(t.numel(), dtype=t.dtype, pin_memory=True) for t in like)
        return tuple(b[:t.numel()].view(t.shape) for b, t in zip(self._cpin, like))


_REC_DTYPE = np.dtype(L.hvn_inst_rec)

_DEFAULT = {}


def _pp(device):
    key = str(device)
    if key not in _DEFAULT:
        _DEFAULT[key] = PostProc(device)
    return _DEFAULT[key]


def process_batch_device(pred_dev, nr_types=None, return_centroids=False, return_contours=False, *, return_features=False, image=None,
                         return_texture=None):
    """pred_dev [N,h,w,3|4] float32 on the GPU -> (inst int32 [N,h,w] device tensor,
    records device tensor | None, counts device tensor | None); with return_contours=True the tuple gains
    `PostProc.contours`' (pts, offs, status) device tensors (None each when there is no record table); records, pts and offs
    in that form are what `viz.overlay_from_records` draws without leaving the device.  return_features=True appends
    `PostProc.features`' tensor as the LAST element (None when there is no record table); `image` (uint8 device tensor
    [N,h,w,3]) adds the colour sums.  return_texture="range" | "fixed" appends `PostProc.texture`'s tensor as the LAST element, after
    the features tensor when both are asked for (None when there is no record table); it needs `image`."""
    if return_texture is not None:
        return_texture = TX.check_scale(return_texture)
        if image is None:
            raise ValueError("return_texture needs the image")
    if image is not None and not return_features and return_texture is None:
        raise ValueError("image is only used with return_features=True or return_texture")
    if image is not None:       # refuse a bad image before anything is launched
        _check_image(image, tuple(pred_dev.shape[:3]), pred_dev.device)
    pp = _pp(pred_dev.device)
    inst = pp.separate(pred_dev)
    out = (inst, None, None)
    if return_centroids or nr_types is not None:
        out = (inst,) + pp.table(inst, pred_dev.contiguous(), nr_types)
    if return_contours:
        out += pp.contours(inst, out[1]) if out[1] is not None else (None, None, None)
    if return_features:
        out += (pp.features(inst, out[1], image) if out[1] is not None else None,)
    if return_texture is not None:
        out += (pp.texture(inst, out[1], image, return_texture) if out[1] is not None else None,)
    return out


def split_contours(pts, offs, n, max_inst):
    """Host arrays of `PostProc.contours` -> one (pts [P,2], offs int64 [max_inst+1]) per map, trace_contours_flat's form."""
    out = []
    for i in range(n):
        o = offs[i * max_inst:(i + 1) * max_inst + 1]
        out.append((pts[int(o[0]):int(o[-1])].copy(), o - o[0]))
    return out


def check_contour_status(status, max_inst):
    """Raises for flagged records (status of `PostProc.contours` on the host); -> True when the points did not fit."""
    if int(status[0]):
        i, j = divmod(int(status[2]), max_inst)
        raise L.HvnError("hvn_trace_contours_device: %d record(s) could not be traced, the first in map %d, label %d: the device "
                         "tracer needs every label to be one 8-connected piece and a record table made from this map "
                         "(trace_contours_flat handles arbitrary maps)" % (int(status[0]), i, j + 1))
    return bool(int(status[1]))


def trace_contours_device(inst_dev, rec_dev):
    """Device counterpart of `trace_contours_flat` for a batch: inst_dev int32 [N,h,w] and rec_dev (`PostProc.table`'s records)
    on the GPU -> a list with one host (pts int32 [P,2], offs int64 [max_inst+1]) per map, exactly what
    trace_contours_flat(inst_host[i], rec_host[i]) returns.  PRECONDITION: every label is one 8-connected piece (the output
    of the instance separation is); a record the device cannot trace raises HvnError naming its map and label.  One host
    synchronisation (a second one in the rare case that the points exceed the default capacity).  The D2H is enqueued before
    the total is known, so it copies `pts` at its whole capacity (N*h*w // 4 points, 2 bytes per pixel), not only the points traced."""
    L.require_gpu()
    pp = _pp(inst_dev.device)
    n, max_inst = rec_dev.shape[0], rec_dev.shape[1]
    max_pts = None
    while True:
        dev = pp.contours(inst_dev, rec_dev, max_pts)
        host = pp._pinned(dev)
        for b, t in zip(host, dev):
            b.copy_(t, non_blocking=True)
        torch.cuda.current_stream(pp.device).synchronize()
        pts, offs, status = (b.numpy() for b in host)
        if not check_contour_status(status, max_inst):
            return split_contours(pts, offs.copy(), n, max_inst)
        max_pts = int(offs[-1])


def trace_contours_flat(inst_host, rec_host):
    """Host: contours[0] of every record (cv2.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE)[0][0] semantics, see
    csrc/hvn_contour.cpp) as flat arrays: (pts int32 [P,2] of (x, y), offs int64 [n_rec + 1]); record i owns
    pts[offs[i]:offs[i+1]] (empty for absent labels).  The flat form is what travels between ranks."""
    inst_host = np.ascontiguousarray(inst_host, np.int32)
    rec_host = np.ascontiguousarray(rec_host)
    h, w = inst_host.shape
    n = rec_host.shape[0]
    # a border pixel is visited at most 4 times (once per 4-neighbour side that faces the background)
    max_pts = 4 * int(rec_host["area"].sum()) + 8 * n + 16
    pts = np.empty((max_pts, 2), np.int32)
    offs = np.empty(n + 1, np.int64)
    tot = L.lib().hvn_trace_contours(inst_host.ctypes.data, h, w, rec_host.ctypes.data, n, pts.ctypes.data, max_pts, offs.ctypes.data)
    if tot < 0:
        raise L.HvnError("hvn_trace_contours failed (%d)" % tot)
    return pts[:tot].copy(), offs


def trace_contours(inst_host, rec_host):
    """-> dict label -> int32 [K,2] array of (x, y) (see trace_contours_flat)."""
    rec_host = np.ascontiguousarray(rec_host)
    pts, offs = trace_contours_flat(inst_host, rec_host)
    return {int(rec_host["label"][i]): pts[offs[i]:offs[i + 1]].copy() for i in range(rec_host.shape[0]) if rec_host["area"][i] > 0}


def records_to_dict(rec_host, nr_types, inst_host=None, contours_flat=None, shift_xy=None, *, feat_host=None, with_colour=False,
                    tex_host=None):
    """One tile's records (numpy structured array) -> the reference's inst_info_dict.  With `inst_host`
    the contours are traced too (or taken from `contours_flat` = trace_contours_flat's result, e.g. traced on another
    rank) and, like the reference (post_proc.py:140-143), instances whose contour
    has fewer than 3 points are left out of the dict (they stay in the instance map).  The per-instance fields are
    computed for the whole tile at once; only the dict assembly is a python loop (a WSI has ~10^6 instances).
    `shift_xy` = (x0, y0): the tile's origin in the slide, added to bbox, centroid and contour the way the WSI merge
    callbacks do (wsi.py:580-584: `+ top_left` with top_left = (x, y) on all three, i.e. x is added to the bbox ROWS --
    the reference's quirk, kept) -- vectorised here instead of three small-array additions per instance there.
    `feat_host` (`features.FEAT_DTYPE` slots parallel to `rec_host`, from `PostProc.features`) adds "features": {...}
    (`features.derive`; the colour entries with `with_colour`) to every entry; they are translation-invariant, `shift_xy` does
    not touch them.  `tex_host` (`texture.TEX_DTYPE` slots parallel to `rec_host`, from `PostProc.texture`) adds "texture": {...}
    (`texture.derive`) likewise."""
    r = rec_host[rec_host["area"] > 0]
    feats = texs = None
    if tex_host is not None:
        tex_host = np.ascontiguousarray(tex_host).view(TX.TEX_DTYPE).reshape(-1)
        if tex_host.shape != rec_host.shape:
            raise ValueError("tex_host %s is not parallel to the records %s" % (tex_host.shape, rec_host.shape))
        texs = TX.to_dicts(TX.derive(tex_host[rec_host["area"] > 0]))
    if feat_host is not None:
        feat_host = np.ascontiguousarray(feat_host).view(F.FEAT_DTYPE).reshape(-1)
        if feat_host.shape != rec_host.shape:
            raise ValueError("feat_host %s is not parallel to the records %s" % (feat_host.shape, rec_host.shape))
        feats = F.to_dicts(F.derive(r, feat_host[rec_host["area"] > 0], with_colour))
    if contours_flat is not None:
        pts, offs = contours_flat
        if shift_xy is not None:
            pts = pts + np.asarray(shift_xy, pts.dtype)
        contours = {int(rec_host["label"][i]): pts[offs[i]:offs[i + 1]] for i in np.nonzero(rec_host["area"] > 0)[0]}
    else:
        contours = trace_contours(inst_host, rec_host) if inst_host is not None else None
    area = r["area"].astype(np.float64)
    bbox = np.stack([np.stack([r["rmin"], r["cmin"]], -1), np.stack([r["rmax"], r["cmax"]], -1)], 1).astype(np.int64)   # [n,2,2]
    # m10/m00 on the crop, then + offset (post_proc.py:145-152)
    cent = np.stack([r["sum_x"] / area + r["cmin"], r["sum_y"] / area + r["rmin"]], -1)
    if shift_xy is not None:
        if contours_flat is None:
            raise ValueError("shift_xy needs contours_flat")
        bbox = bbox + np.asarray(shift_xy, bbox.dtype)
        cent = cent + np.asarray(shift_xy, cent.dtype)
    labels = r["label"].tolist()
    types = r["type"].tolist() if nr_types is not None else None
    tprob = (r["type_count"] / (area + 1.0e-6)).tolist() if nr_types is not None else None
    out = {}
    for i, lab in enumerate(labels):
        contour = None
        if contours is not None:
            contour = contours[lab]
            if contour.shape[0] < 3:
                continue
        out[lab] = {"bbox": bbox[i], "centroid": cent[i], "contour": contour,
                    "type_prob": None if tprob is None else tprob[i], "type": None if types is None else types[i]}
        if feats is not None:
            out[lab]["features"] = feats[i]
        if texs is not None:
            out[lab]["texture"] = texs[i]
    return out


def process(pred_map, nr_types=None, return_centroids=False, contours="host", *, features=False, image=None, neighbours=None, clusters=None,
            texture=None):
    """Reference signature (post_proc.py:94): one host map [H,W,3|4] float32.  contours="device" traces the contours on
    the GPU (`trace_contours_device`) instead of on the host; the result is the same.  features=True adds "features" to every
    entry of the dict (`features.derive`; it implies return_centroids); `image` (host uint8 [H,W,3], RGB) adds mean_rgb / std_rgb.
    neighbours / clusters: the point-pattern analyses of hover_net_amd/points.py on the finished dict, on the GPU (they imply
    return_centroids).  texture=True | "range" | "fixed" (True means "range") adds "texture" to every entry of the dict
    (`texture.derive` of `PostProc.texture`'s counts; it implies return_centroids); it needs `image` and raises ValueError before
    any launch without one."""
    from . import points as PT
    from . import clusters as CL
    from . import neighbours as NB

    if contours not in ("host", "device"):
        raise ValueError('contours must be "host" or "device", got %r' % (contours,))
    specs = PT.resolve_specs(neighbours, clusters, typed=nr_types is not None)
    return_centroids = return_centroids or specs.any_annotation
    img_dev = None
    if texture is not None:
        texture = TX.check_scale(texture)
        if image is None:
            raise ValueError("texture needs the image")
    if image is not None:
        if not features and texture is None:
            raise ValueError("image is only used with features=True or texture")
        image = np.asarray(image)
        if image.dtype != np.uint8:
            raise TypeError("image must be uint8, got %s" % image.dtype)
        if image.shape != tuple(np.shape(pred_map)[:2]) + (3,):
            raise ValueError("image %s does not match the map: expected %s" % (image.shape, tuple(np.shape(pred_map)[:2]) + (3,)))
        img_dev = torch.from_numpy(np.ascontiguousarray(image)).unsqueeze(0).to("cuda")
    pred = torch.from_numpy(np.ascontiguousarray(pred_map, np.float32)).unsqueeze(0).to("cuda")
    inst, rec, _ = process_batch_device(pred, nr_types, return_centroids or features or texture is not None)
    feat = _pp(pred.device).features(inst, rec, img_dev) if features and rec is not None else None
    tex = _pp(pred.device).texture(inst, rec, img_dev, texture) if texture is not None and rec is not None else None
    flat = trace_contours_device(inst, rec)[0] if rec is not None and contours == "device" else None
    pred_inst = inst[0].cpu().numpy()
    info = None
    if rec is not None:
        info = records_to_dict(rec[0].cpu().numpy().view(_REC_DTYPE).reshape(-1), nr_types, pred_inst, contours_flat=flat,
                               feat_host=None if feat is None else feat[0].cpu().numpy(), with_colour=image is not None,
                               **({} if tex is None else {"tex_host": tex[0].cpu().numpy()}))
        PT.annotate(info, specs, nr_types, pred.device)
    return pred_inst, info
