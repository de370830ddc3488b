"""Validation statistics accumulated on the device: the scalars of `run_desc.proc_valid_step_output` (np_acc, np_dice,
tp_dice_<t>, hv_mse -- the scalar half of the reference's models/hovernet/run_desc.py:262-333) without keeping a single raw array.

Every scalar is a ratio of integer counts or a sum of squares over a pixel count, so an epoch is a state of `4 + 2 * nr_types`
int64 counts and one float64: `update` adds a batch to it with one launch pair (csrc/hvn_valid.hip) on the current stream and no host
sync, `merge_ranks` makes it the state of the whole validation set on every rank, `scalars` copies it to the host once and does
the divisions there, with `proc_valid_step_output`'s own float64 expressions.  The counts are exact, so np_acc and the Dice scores
equal the host path's bit for bit; hv_mse is the same non-negative float64 terms added in another (fixed) order.

Nothing here keeps predictions, targets or images.  The epoch's picture (the "image" half of `proc_valid_step_output`, the
reference's visualisation of eight validation patches) does not need them either: `plan_viz` names the samples of the coming epoch
to draw, and `update` draws each of them that falls into its batch straight into its block of one device strip (`viz.strip_device`,
one more launch); `track` brings scalars and strip to the host in one copy.
"""
import numpy as np
import torch

from . import lib as L

MAX_TYPES = 16      # the kernel's cap on nr_types


def launch(pred, np_map, hv_map, tp_map, shape, nr_types, counts, hv_sse, workspace):
    """`hvn_valid_stats` (include/hvn.h) on device tensors, on the current stream of `counts`' device: adds the batch of
    `shape` = (n, h, w, c) to `counts` / `hv_sse`.  No sync.  Whatever the library refuses raises HvnError with the state untouched."""
    n, h, w, c = (int(v) for v in shape)
    with torch.cuda.device(counts.device):
        L.call("hvn_valid_stats", pred.data_ptr(), np_map.data_ptr(), hv_map.data_ptr(), None if tp_map is None else tp_map.data_ptr(), n, h, w, c,
               int(nr_types), counts.data_ptr(), hv_sse.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
               L.stream_ptr(counts.device))


class ValidStats:
    """`counts` (int64: pixels, np_correct, np_inter, np_total, then tp_inter_t, tp_total_t per type) and `hv_sse` (float64 [1]) are
    views of one buffer on `device`.  Only `update` needs a GPU: a CPU state can be filled by hand, merged and read."""

    def __init__(self, nr_types=None, device="cuda"):
        self.nr_types = None if nr_types is None else int(nr_types)
        nt = self.nr_types or 0
        if self.nr_types is not None and not 0 < nt <= MAX_TYPES:
            raise ValueError("nr_types must be None or in [1, %d]" % MAX_TYPES)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._buf = torch.zeros(4 + 2 * nt + 1, dtype=torch.int64, device=self.device)
        self.counts = self._buf[:-1]
        self.hv_sse = self._buf[-1:].view(torch.float64)
        self._ws = None
        self._plan, self._img_hw, self._strip, self._drawn, self._seen = None, None, None, None, 0
        self.viz_missing = 0

    def reset(self):
        """Clear the counts, the plan of `plan_viz` and its strip: the next epoch draws nothing unless it is planned again."""
        self._buf.zero_()
        self._plan, self._img_hw, self._strip, self._drawn, self._seen = None, None, None, None, 0

    def plan_viz(self, indices, img_hw=None):
        """Draw the samples `indices` of the epoch that starts now: positions in this rank's sample sequence (the order in which
        `update` sees them, counted from 0 at the last `reset`), any order, duplicates allowed.  Block j of the strip is sample
        indices[j].  `img_hw`: the (height, width) the feed's images must have, checked in `update` (None: not checked).  A
        planned index the epoch never reaches leaves its block zero and is counted in `viz_missing` by `track`."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        if (idx < 0).any():
            raise ValueError("plan_viz: negative sample index")
        if self._seen:
            raise ValueError("plan_viz after the epoch's first update: call it after reset()")
        self._plan = idx
        self._img_hw = None if img_hw is None else (int(img_hw[0]), int(img_hw[1]))
        self._drawn = np.zeros(idx.shape[0], bool)
        self._strip = None

    def _draw(self, pred_dev, feed, np_map, hv_map, tp_map):
        from . import viz

        n, h, w, _c = (int(v) for v in pred_dev.shape)
        img = torch.as_tensor(feed["img"])
        if self._img_hw is not None and tuple(int(v) for v in img.shape[1:3]) != self._img_hw:
            raise ValueError("plan_viz was told images of %s, the feed's are %s" % (self._img_hw, tuple(img.shape[1:3])))
        typed = self.nr_types is not None       # `launch` has refused a typed state without type truths
        if self._strip is None and self._plan.shape[0]:
            self._strip = torch.zeros((self._plan.shape[0] * 2 * h, (5 if typed else 4) * w, 3), dtype=torch.uint8, device=self.device)
        hit = np.nonzero((self._plan >= self._seen) & (self._plan < self._seen + n))[0]
        if hit.size:
            sel = np.stack([self._plan[hit] - self._seen, hit], 1)
            viz.strip_device(img.to(self.device, torch.uint8, non_blocking=True).contiguous(), pred_dev, np_map, hv_map, tp_map, sel,
                             out=self._strip, nr_types=self.nr_types)
            self._drawn[hit] = True

    def _feed(self, x, dtype, shape):
        return torch.as_tensor(x).to(self.device, dtype, non_blocking=True).reshape(shape).contiguous()

    def update(self, pred_dev, feed):
        """Add one batch: `pred_dev` = float32 device tensor [N,h,w,3|4] as `run_desc.infer_step_device` returns it (read in place),
        `feed` = the loader's dict (np_map, hv_map, tp_map with types; device tensors, or host tensors / arrays, which are uploaded).
        Launches on the current stream and returns without a host sync; the launches read `pred_dev` in stream order, so the next
        engine run on the same stream may overwrite the buffer it aliases."""
        if self.device.type != "cuda":
            raise L.HvnError("ValidStats.update needs a device state (there is no CPU fallback for the kernel)")
        if not (torch.is_tensor(pred_dev) and pred_dev.is_cuda and pred_dev.dtype == torch.float32 and pred_dev.dim() == 4
                and pred_dev.is_contiguous() and pred_dev.device == self.device):
            raise L.HvnError("ValidStats.update: pred_dev must be a contiguous float32 [N,h,w,C] tensor on %s" % self.device)
        n, h, w, c = (int(v) for v in pred_dev.shape)
        np_map = self._feed(feed["np_map"], torch.int32, (n, h, w))
        hv_map = self._feed(feed["hv_map"], torch.float32, (n, h, w, 2))
        tp_map = None
        if self.nr_types is not None and feed.get("tp_map") is not None:
            tp_map = self._feed(feed["tp_map"], torch.int32, (n, h, w))
        self._ws = L.grown(self._ws, max(int(L.lib().hvn_valid_stats_workspace_bytes(n, h, w)), 1), self.device)
        launch(pred_dev, np_map, hv_map, tp_map, (n, h, w, c), self.nr_types or 0, self.counts, self.hv_sse, self._ws)
        if self._plan is not None:
            self._draw(pred_dev, feed, np_map, hv_map, tp_map)
        self._seen += n

    def merge_ranks(self):
        """Make the state the whole validation set's on every rank.  A collective: EVERY rank of the process group must call it, once
        per epoch, also a rank whose shard was empty.  Without an initialised torch.distributed group of more than one rank it
        does nothing.  The counts are SUM-all-reduced as int64 (exact); the per-rank hv_sse values are all-gathered and added in rank
        order on every rank, so the sum does not depend on the backend's reduction order and every rank holds the same bits."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        dev = self.device if dist.get_backend() == "nccl" else torch.device("cpu")
        counts = self.counts.to(dev, copy=True)
        sse = self.hv_sse.to(dev, copy=True)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        parts = [torch.empty_like(sse) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, sse)
        total = parts[0]
        for p in parts[1:]:
            total = total + p
        self.counts.copy_(counts)
        self.hv_sse.copy_(total)

    def _scalars_of(self, host):
        c, hv_sse = host[:-1], host[-1:].view(np.float64)[0]
        nr_pixels = int(c[0])

        def dice(inter, total):
            return 2.0 * inter / (total + 1.0e-8)

        out = {"np_acc": c[1] / nr_pixels, "np_dice": dice(c[2], c[3])}
        for type_id in range(self.nr_types or 0):
            out["tp_dice_%d" % type_id] = dice(c[4 + 2 * type_id], c[5 + 2 * type_id])
        out["hv_mse"] = hv_sse / nr_pixels
        return out

    def scalars(self):
        """The dict of `proc_valid_step_output(...)["scalar"]` from one device-to-host copy of the state."""
        return self._scalars_of(self._buf.cpu().numpy())

    def track(self):
        """`proc_valid_step_output`'s dict.  Without a plan "image" is empty; with one (and at least one `update`) it holds the strip
        under "output", and state and strip come to the host in ONE copy.  The strip is this rank's: `merge_ranks` does not touch it."""
        if self._plan is None or self._strip is None:
            self.viz_missing = 0 if self._plan is None else int(self._plan.shape[0])
            return {"scalar": self.scalars(), "image": {}}
        nb = self._buf.numel() * 8
        host = torch.cat([self._buf.view(torch.uint8), self._strip.reshape(-1)]).cpu().numpy()
        self.viz_missing = int((~self._drawn).sum())
        return {"scalar": self._scalars_of(host[:nb].view(np.int64)), "image": {"output": host[nb:].reshape(tuple(self._strip.shape)).copy()}}
