"""Drop-in for `models.hovernet.run_desc.infer_step`
(/root/reference/models/hovernet/run_desc.py:171-197).

Same signature and return contract -- `infer_step(batch_data, model)` with `batch_data`
a uint8 `[N,H,W,3]` tensor, returning a float32 numpy array `[N,h,w,3|4]` =
`[type?, p_nuc, h, v]` on the host -- but the uint8 bytes go straight to HBM (no float
NCHW copy), the whole forward + softmax/argmax/concat epilogue is one launch plan, and
the only host sync is the final D2H of the 102 KB/tile map.

`train_step` / `valid_step` (run_desc.py:12-167) run the training-mode forward, the losses, the backward pass
and the optimizer step on the HIP path (hover_net_amd.train_engine).  `valid_step_stats` is `valid_step` with the
epoch's statistics accumulated on the device (hover_net_amd.valid_stats) instead of raw arrays on the host.

`viz_step_output` (run_desc.py:201-256) is the run loop's picture on the host, numpy only; `viz_step_output_device` draws the same
bytes on the device (hover_net_amd.viz, csrc/hvn_viz.hip) from device tensors.

`infer_step_device` is the same step without the D2H: it returns the device tensor so
`post_proc.process_batch_device` can run the instance separation on-GPU with no CPU
round trip per tile (the north-star path; bench.py times this one).
"""
import torch


def _unwrap(model):
    return model.module if hasattr(model, "module") and not hasattr(model, "engine") else model


def infer_step_device(batch_data, model, tta=None):
    """uint8 [N,H,W,3] (host or device) -> float32 device tensor [N,h,w,3|4]; aliases an
    engine buffer that the next call overwrites.  tta: None, or a view set of hover_net_amd.tta ("flips", "rot", "d4" or a tuple of
    view ids): the map is then the mean over the views' outputs mapped back, the type that of the mean probabilities
    (`Engine.run_tta`)."""
    if tta is not None:
        from . import tta as TT

        tta = TT.views(tta)         # ValueError before anything is launched
    net = _unwrap(model)
    net.eval()
    if batch_data.dtype != torch.uint8:
        batch_data = batch_data.to(torch.uint8)
    dev = next(net.parameters()).device
    imgs = batch_data.to(dev, non_blocking=True)
    eng = net.engine(imgs.shape[0])
    _, pred = eng.run(imgs) if tta is None else eng.run_tta(imgs, tta)
    return pred


def infer_step(batch_data, model, tta=None):
    pred = infer_step_device(batch_data, model, tta)
    return pred.cpu().numpy()


def _dist():
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist
    return None


def train_step(batch_data, run_info):
    """Drop-in for run_desc.py:12-109.  Same protocol: `run_info = [{"net": {"desc", "optimizer", "extra_info"}},
    state]`, `batch_data` = the loader's dict (img uint8 NHWC, np_map, hv_map, tp_map?), returns
    `{"EMA": {loss_<branch>_<term>, overall_loss}, "raw": {img, np: (true, pred), hv: (true, pred)}}`.  "raw" holds host arrays of
    two random samples (five copies to the host per step); with `extra_info["viz"] == "device"` it holds device tensors of the same
    two samples instead and the step copies nothing (`viz_step_output_device`, `run_engine.VisualizeOutput` draw from them).

    What runs: forward in train() mode (batch-statistics BatchNorm, running stats updated), the reference's loss
    set (np bce+dice, hv mse+msge, tp bce+dice) with the weights of `extra_info["loss"]` (opt.py:47-51), backward
    and `optimizer.step()`, all on the HIP path (hover_net_amd.train_engine).  Multi-GPU is one process per GPU:
    when torch.distributed is initialised the loss partial sums and the flat gradient slab are SUM-all-reduced
    (RCCL), which reproduces the reference's single-process DataParallel step over the concatenated batch
    (full-batch dice / msge denominators, per-replica BatchNorm statistics)."""
    from . import train_engine

    run_info, _state_info = run_info
    model = run_info["net"]["desc"]
    optimizer = run_info["net"]["optimizer"]
    net = _unwrap(model)
    loss_opts = run_info["net"].get("extra_info", {}).get("loss")
    if loss_opts is not None:       # the branches the network does not have are ignored, like run_desc.py:66 (`for branch_name in pred_dict`)
        loss_opts = {k: dict(v) for k, v in loss_opts.items() if k in ("np", "hv") or (k == "tp" and net.nr_types is not None)}
    imgs = batch_data["img"]
    eng = train_engine.engine_for(net, imgs.shape[0])
    net.train()
    eng.set_loss_weights(loss_opts)
    eng.load_batch(batch_data)
    eng.forward()
    dist = _dist()
    if dist is None:
        eng.loss_and_backward()
    else:
        eng.loss_and_backward(world=dist.get_world_size(),
                              all_reduce=lambda t, async_op=False: dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=async_op))
    optimizer.step()
    result = {"EMA": dict(eng.loss_terms())}
    # two random samples for the visualisation protocol (run_desc.py:90-107)
    idx = torch.randint(0, imgs.shape[0], (2,))
    if run_info["net"].get("extra_info", {}).get("viz") == "device":
        # the same two draws, gathered on the engine's stream and kept on the device: no copy to the host, no sync.  Cloned, because
        # the logits alias engine buffers that the next step overwrites.
        dev = eng.device
        didx = idx.to(dev, non_blocking=True)

        def pick(t, dtype):
            t = torch.as_tensor(t)          # a host feed is indexed on the host: two samples travel, not the batch
            t = t.index_select(0, didx) if t.is_cuda else t[idx].to(dev, non_blocking=True)
            return t.type(dtype).contiguous()

        prob_np = torch.softmax(eng.logits["np"].index_select(0, didx), 1)[:, 1].clone()
        pred_hv = eng.logits["hv"].index_select(0, didx).permute(0, 2, 3, 1).contiguous()
        result["raw"] = {"img": pick(imgs, torch.uint8), "np": (pick(batch_data["np_map"], torch.int64), prob_np),
                         "hv": (pick(batch_data["hv_map"], torch.float32), pred_hv)}
        return result
    didx = idx.to(eng.device)
    prob_np = torch.softmax(eng.logits["np"][didx], 1)[:, 1].cpu().numpy()
    pred_hv = eng.logits["hv"][didx].permute(0, 2, 3, 1).cpu().numpy()
    true_np = torch.as_tensor(batch_data["np_map"])[idx].type(torch.int64).cpu().numpy()      # .cpu(): the feed may already live on the device
    true_hv = torch.as_tensor(batch_data["hv_map"])[idx].type(torch.float32).cpu().numpy()
    result["raw"] = {"img": torch.as_tensor(imgs)[idx].byte().cpu().numpy(), "np": (true_np, prob_np), "hv": (true_hv, pred_hv)}
    return result


def valid_step(batch_data, run_info):
    """Drop-in for run_desc.py:113-167: eval-mode forward of a validation batch on the HIP path; returns
    the same `{"raw": {...}}` protocol (prob_np = softmax(np)[..., 1], pred_hv, argmax type map)."""
    run_info, _state_info = run_info
    model = run_info["net"]["desc"]
    net = _unwrap(model)
    imgs = batch_data["img"]
    true_np = torch.squeeze(batch_data["np_map"]).type(torch.int64).cpu()        # .cpu(): a device-resident feed (augment.DevicePatchLoader) is fine too
    true_hv = torch.squeeze(batch_data["hv_map"]).type(torch.float32).cpu()
    pred = infer_step_device(imgs, model)            # [N,h,w,3|4] = [type?, p_nuc, h, v] on the device
    pred = pred.cpu()
    c0 = 0 if net.nr_types is None else 1
    result = {"raw": {"imgs": imgs.cpu().numpy(), "true_np": true_np.numpy(), "true_hv": true_hv.numpy(),
                      "prob_np": pred[..., c0].numpy().copy(), "pred_hv": pred[..., c0 + 1:c0 + 3].numpy().copy()}}
    if net.nr_types is not None:
        result["raw"]["true_tp"] = torch.squeeze(batch_data["tp_map"]).type(torch.int64).cpu().numpy()
        result["raw"]["pred_tp"] = pred[..., 0].numpy().copy()
    return result


def valid_step_stats(batch_data, run_info):
    """`valid_step` with the statistics kept on the device: the eval-mode forward, then `run_info["valid_stats"]` (a
    `valid_stats.ValidStats`, next to "net" in the valid engine's run_info) adds the batch to its state on the same stream --
    no copy to the host, no sync, nothing accumulated: "raw" is empty, and `ValidStats.track()` at the end of the epoch gives
    what `proc_valid_step_output` gives over the accumulated `valid_step` outputs (`run_engine.DeviceValidStats`)."""
    run_info, _state_info = run_info
    pred = infer_step_device(batch_data["img"], run_info["net"]["desc"])     # aliases an engine buffer: read before the next run
    run_info["valid_stats"].update(pred, batch_data)
    return {"raw": {}}


def _aligned_shape(imgs, true_np, pred_np):
    """run_desc.py:213-214: the smallest height and width among img, true_np and pred_np.  The reference stacks the three shapes
    into one array, which numpy >= 1.24 refuses unless the maps carry a channel axis ([n,h,w,1]); here [n,h,w] maps are fine too."""
    import numpy as np

    return np.min(np.array([list(imgs.shape[:3]), list(true_np.shape[:3]), list(pred_np.shape[:3])]), axis=0)[1:3]


def viz_step_output(raw_data, nr_types=None):
    """Drop-in for run_desc.py:201-256, numpy only: `raw_data` = {"img": [n,ih,iw,3], "np": (true, pred), "hv": (true, pred), "tp":
    (true, pred) with `nr_types`} -> uint8 [n * 2h, ncol * w, 3]: per sample a row of truths above a row of predictions, each the
    image cropped at its centre to the `aligned_shape` of the reference, then NP over 0..1, H and V over -1..1 and TP over
    0..nr_types through `viz.colorize`.  This host function is the definition of the picture; the device forms are held to it."""
    import numpy as np

    from . import viz

    imgs = raw_data["img"]
    true_np, pred_np = raw_data["np"]
    true_hv, pred_hv = raw_data["hv"]
    if nr_types is not None:
        true_tp, pred_tp = raw_data["tp"]
    ah, aw = (int(v) for v in _aligned_shape(imgs, true_np, pred_np))

    def colorize(ch, vmin, vmax):       # a map of height or width 1 keeps its two axes (the reference's squeeze loses them)
        return viz.colorize(ch, vmin, vmax).reshape(ch.shape[0], ch.shape[1], 3)

    rows = []
    for idx in range(imgs.shape[0]):
        h0, w0 = int((imgs[idx].shape[0] - ah) * 0.5), int((imgs[idx].shape[1] - aw) * 0.5)
        img = imgs[idx][h0:h0 + ah, w0:w0 + aw]
        true_row = [img, colorize(true_np[idx], 0, 1), colorize(true_hv[idx][..., 0], -1, 1), colorize(true_hv[idx][..., 1], -1, 1)]
        pred_row = [img, colorize(pred_np[idx], 0, 1), colorize(pred_hv[idx][..., 0], -1, 1), colorize(pred_hv[idx][..., 1], -1, 1)]
        if nr_types is not None:
            true_row.append(colorize(true_tp[idx], 0, nr_types))
            pred_row.append(colorize(pred_tp[idx], 0, nr_types))
        rows.append(np.concatenate([np.concatenate(true_row, axis=1), np.concatenate(pred_row, axis=1)], axis=0))
    return np.concatenate(rows, axis=0)


def viz_step_output_device(raw_data, nr_types=None):
    """`viz_step_output` for a `raw_data` of device tensors (what `train_step` returns with `extra_info["viz"] == "device"`): the same
    bytes as a uint8 device tensor, from torch packing and one `hvn_viz_strip` launch on the current stream, no host sync.  The
    truths of NP and TP must be integer (or bool) tensors -- they travel as int32 --, and the truth and prediction maps of one
    size that the image covers (the only shapes the reference's concatenation accepts)."""
    from . import viz

    imgs = raw_data["img"]
    true_np, pred_np = raw_data["np"]
    true_hv, pred_hv = raw_data["hv"]
    tensors = [imgs, true_np, pred_np, true_hv, pred_hv]
    if nr_types is not None:
        true_tp, pred_tp = raw_data["tp"]
        tensors += [true_tp, pred_tp]
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise ValueError("viz_step_output_device takes device tensors (viz_step_output draws host arrays)")
    n = int(imgs.shape[0])
    if imgs.dim() != 4 or imgs.shape[-1] != 3 or n == 0:
        raise ValueError("img must be [n, ih, iw, 3] with n > 0, got %s" % (tuple(imgs.shape),))
    pred_np = pred_np.reshape(n, *pred_np.shape[1:3])
    h, w = int(pred_np.shape[1]), int(pred_np.shape[2])

    def truth(t, what):
        if t.dtype.is_floating_point or t.dtype.is_complex:
            raise ValueError("%s must be an integer tensor, got %s" % (what, t.dtype))
        return t.reshape(n, h, w).to(torch.int32).contiguous()

    planes = [pred_np.to(torch.float32), pred_hv.reshape(n, h, w, 2).to(torch.float32)[..., 0], pred_hv.reshape(n, h, w, 2).to(torch.float32)[..., 1]]
    tp_map = None
    if nr_types is not None:
        planes.insert(0, pred_tp.reshape(n, h, w).to(torch.float32))
        tp_map = truth(true_tp, "the true type map")
    sel = [(i, i) for i in range(n)]
    return viz.strip_device(imgs.to(torch.uint8).contiguous(), torch.stack(planes, -1).contiguous(), truth(true_np, "the true nucleus map"),
                            true_hv.reshape(n, h, w, 2).to(torch.float32).contiguous(), tp_map, sel, n_blocks=n, nr_types=nr_types)


def proc_valid_step_output(raw_data, nr_types=None, *, image=False, selected_idx=None):
    """run_desc.py:262-344: validation statistics over the accumulated `valid_step` outputs (`raw_data[name]` = list of per-patch
    arrays or one stacked array): nucleus-pixel accuracy and Dice at p > 0.5, per-type Dice, HV mean squared error per pixel.  Host
    numpy, computed over the whole set at once instead of patch by patch.
    `image=True` adds the picture half the way run_desc.py:328-342 does: `track["image"]["output"]` = `viz_step_output` of eight
    patches drawn with `np.random.randint(0, len(imgs), size=(8,))` (the global numpy stream, like the reference), or of
    `selected_idx`.  The default leaves "image" empty and draws no random number."""
    import numpy as np

    track = {"scalar": {}, "image": {}}
    prob_np = np.asarray(raw_data["prob_np"])
    true_np = np.asarray(raw_data["true_np"])
    pred_np = (prob_np > 0.5).astype(np.int32)

    def dice(true, pred, label):
        t, p = (true == label), (pred == label)
        return 2.0 * np.logical_and(t, p).sum() / (t.sum() + p.sum() + 1.0e-8)

    nr_pixels = true_np.size
    track["scalar"]["np_acc"] = (pred_np == true_np).sum() / nr_pixels
    track["scalar"]["np_dice"] = dice(true_np, pred_np, 1)
    if nr_types is not None:
        pred_tp, true_tp = np.asarray(raw_data["pred_tp"]), np.asarray(raw_data["true_tp"])
        for type_id in range(nr_types):
            track["scalar"]["tp_dice_%d" % type_id] = dice(true_tp, pred_tp, type_id)
    err = np.asarray(raw_data["pred_hv"], np.float64) - np.asarray(raw_data["true_hv"], np.float64)
    track["scalar"]["hv_mse"] = (err * err).sum() / nr_pixels
    if image:
        imgs = raw_data["imgs"]
        if selected_idx is None:
            selected_idx = np.random.randint(0, len(imgs), size=(8,)).tolist()

        def take(x):
            return np.array([x[idx] for idx in selected_idx])

        viz_raw = {"img": take(imgs), "np": (take(true_np), take(prob_np)), "hv": (take(raw_data["true_hv"]), take(raw_data["pred_hv"]))}
        if nr_types is not None:
            viz_raw["tp"] = (take(true_tp), take(pred_tp))
        track["image"]["output"] = viz_step_output(viz_raw, nr_types)
    return track
