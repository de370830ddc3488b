"""Two-stream tile pipeline: the instance separation of batch i runs on a side HIP stream while the
network of batch i+1 runs on the main stream.

The reference overlaps these two stages with a CPU process pool next to the GPU loop
(/root/reference/infer/tile.py:232-234, 361-386).  Here both stages are on the GPU: the network
saturates the matrix cores, the post-processing is a chain of small latency-bound launches (its
watershed uses one workgroup per tile), so running them concurrently hides the latter almost entirely.
Hand-over is a 3.3 MB device copy of the prediction maps into one of two ping-pong buffers, ordered with
HIP events (no host sync anywhere in `submit`).
"""
import torch

from . import post_proc, run_desc


class TilePipeline:
    def __init__(self, model, nr_types=None, return_centroids=True, device=None, contours=False, contour_max_pts=None, *, tta=None):
        """tta: None, or a view set of hover_net_amd.tta: every `submit` then runs the test-time-augmented step (`Engine.run_tta`).
        contours=True: every batch's contours are traced on the side stream too (`PostProc.contours`; the instance
        separation's labels are one piece each, which is what the device tracer needs) and `submit` returns
        (inst, records, counts, pts, offs, status).  contour_max_pts: capacity of `pts` per batch (default: a quarter of the
        batch's pixels); a batch that needs more is traced again with the exact size in `wait()`.  With to_host=True the whole
        `pts` buffer is copied at that capacity (2 bytes per pixel by default), whatever part of it the batch's points fill."""
        from . import tta as TT

        self.model = model
        self.tta = TT.views(tta)
        self.nr_types = nr_types
        self.return_centroids = return_centroids
        self.contours = bool(contours)
        self.contour_max_pts = contour_max_pts
        if self.contours and not (return_centroids or nr_types is not None):
            raise ValueError("contours=True needs the record table (return_centroids or nr_types)")
        self._pending = []                           # contours=True: (device result, returned result) of the batches since the last wait()
        net = model.module if hasattr(model, "module") and not hasattr(model, "engine") else model
        self.device = torch.device(device) if device is not None else next(net.parameters()).device
        self.side = torch.cuda.Stream(self.device)
        self._pp = post_proc.PostProc(self.device)   # own workspace: used on the side stream only
        self._buf = [None, None]
        self._free = [None, None]                    # event: the side stream is done reading _buf[k]
        self._n = 0
        self._last = None
        # host batches (the reference contract: infer_step takes a CPU uint8 tensor) go up on their own copy stream into one of
        # two device slots, so the H2D of batch i+1 runs under the network of batch i
        self.h2d = torch.cuda.Stream(self.device)
        self._in = [None, None]
        self._in_free = [None, None]                 # event: the network is done reading _in[k]
        # optional diagnosis (bench.py --gpus N): HIP events around every `gather` call on the side stream
        self.time_gather = False
        self.gather_events = []

    def submit(self, tiles_u8, extra_maps=None, gather=None, to_host=False):
        """Network on the current stream, post-processing on the side stream.  Returns
        (inst, records, counts) tensors that are valid after `wait()` (or after the side
        stream is otherwise synchronised).  `extra_maps`: optional additional [N,h,w,C] maps to
        post-process in the same side-stream slot (bench.py's structured workload).
        `gather`: optional callable applied to the result tuple on the side stream (the multi-GPU
        path hands `infer_tile.gather_to_rank0` here, so the RCCL gather overlaps the next network
        pass too).  `to_host=True`: the results are copied to pinned host memory on the side stream
        (the reference's contract ends on the host: infer/tile.py:308-316); the returned tensors are
        then the pinned buffers of this slot, overwritten two submits later.
        With contours=True the tuple is (inst, records, counts, pts, offs, status); `status` is checked in `wait()`, not here:
        `submit` never waits on the host."""
        if self.contours and gather is not None:
            raise ValueError("contours=True does not go through a gather: the multi-GPU paths carry host contour arrays")
        main = torch.cuda.current_stream(self.device)
        k = self._n & 1
        self._n += 1
        if not tiles_u8.is_cuda:
            tiles_u8 = self._upload(tiles_u8, k, main)
        pred = run_desc.infer_step_device(tiles_u8, self.model, **({"tta": self.tta} if self.tta is not None else {}))       # aliases the engine's buffer
        if self._in[k] is not None and tiles_u8 is self._in[k]:
            self._in_free[k] = torch.cuda.Event()
            self._in_free[k].record(main)
        if self._free[k] is not None:
            main.wait_event(self._free[k])                             # ping-pong slot k is free again
        if self._buf[k] is None or self._buf[k].shape != pred.shape:
            self._buf[k] = torch.empty_like(pred)
        self._buf[k].copy_(pred)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            out = self._run_pp(self._buf[k])
            if extra_maps is not None:
                out = self._run_pp(extra_maps)
            if gather is not None:
                if self.time_gather:
                    g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    g0.record(self.side)
                out = gather(out)
                if self.time_gather:
                    g1.record(self.side)
                    self.gather_events.append((g0, g1))
            dev = out
            if to_host and out is not None:
                out = self._to_host(out, k)
            if self.contours:
                self._pending.append((dev, out))
            self._free[k] = torch.cuda.Event()
            self._free[k].record(self.side)
        self._last = out
        return out

    def _upload(self, tiles_host, k, main):
        if tiles_host.dtype != torch.uint8:
            tiles_host = tiles_host.to(torch.uint8)
        if self._in[k] is None or self._in[k].shape != tiles_host.shape:
            self._in[k] = torch.empty(tiles_host.shape, dtype=torch.uint8, device=self.device)
            self._in_free[k] = None
        with torch.cuda.stream(self.h2d):
            if self._in_free[k] is not None:
                self.h2d.wait_event(self._in_free[k])
            self._in[k].copy_(tiles_host, non_blocking=True)          # asynchronous when the source is pinned
            up = torch.cuda.Event()
            up.record(self.h2d)
        main.wait_event(up)
        return self._in[k]

    def _run_pp(self, maps):
        inst = self._pp.separate(maps)
        if self.return_centroids or self.nr_types is not None:
            rec, counts = self._pp.table(inst, maps, self.nr_types)
            if self.contours:
                return (inst, rec, counts) + self._pp.contours(inst, rec, self.contour_max_pts)
            return inst, rec, counts
        return inst, None, None

    def _to_host(self, out, k):
        """D2H of (inst, records, counts) into this slot's pinned buffers, asynchronous on the side stream."""
        if not hasattr(self, "_pin"):
            self._pin = [None, None]
        bufs = self._pin[k]
        if bufs is None or any((b is None) != (t is None) or (t is not None and (b.shape != t.shape or b.dtype != t.dtype))
                               for b, t in zip(bufs, out)):
            bufs = tuple(None if t is None else torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in out)
            self._pin[k] = bufs
        for b, t in zip(bufs, out):
            if t is not None:
                b.copy_(t, non_blocking=True)
        return bufs

    def flood_stats(self):
        """Replay statistics of the watershed of the last network output this pipeline post-processed (waits for the side stream)."""
        self.side.synchronize()
        return self._pp.flood_stats(self.side)

    def gather_ms(self):
        """Mean duration (ms) of the timed `gather` calls since the last call of this method (side stream synchronised first)."""
        self.side.synchronize()
        ev, self.gather_events = self.gather_events, []
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev) if ev else 0.0

    def wait(self):
        self.side.synchronize()
        if self._pending:
            self._check_contours()
        return self._last

    def _check_contours(self):
        """contours=True: the status words of the batches since the last wait().  A flagged record raises; a batch whose points
        did not fit is traced again with the exact size, and the new points replace the old IN the tensors `submit` returned.
        Status and total are read from each batch's own device tensors, never from the pinned buffers: with to_host=True a
        slot's pinned buffers hold only the NEWEST batch submitted to that slot, so an older batch of the slot is checked for
        flags only (its host copy is gone, as `submit` says) and only the newest one is traced again and copied."""
        pending, self._pending = self._pending, []
        newest = {id(out[3]): i for i, (dev, out) in enumerate(pending) if out is not dev}   # per pinned buffer
        with torch.cuda.stream(self.side):
            status = torch.stack([dev[5] for dev, _ in pending]).cpu().numpy()
            totals = torch.stack([dev[4][-1] for dev, _ in pending]).cpu().tolist()
        for i, (dev, out) in enumerate(pending):
            if not post_proc.check_contour_status(status[i], dev[1].shape[1]):
                continue
            if out is not dev and newest[id(out[3])] != i:
                continue
            with torch.cuda.stream(self.side):
                pts, offs, st = self._pp.contours(dev[0], dev[1], int(totals[i]))
                for old, new in ((dev[3], pts), (dev[5], st)) + (((out[3], pts), (out[5], st)) if out is not dev else ()):
                    old.resize_(new.shape).copy_(new)    # offs is exact already
                self.side.synchronize()
