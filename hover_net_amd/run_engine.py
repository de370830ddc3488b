"""The run-loop protocol of the reference (`run_utils/engine.py:132-204` RunEngine / Events / State and the data-path callbacks
of `run_utils/callbacks/base.py`): an engine walks a dataloader, calls `run_step(batch, [run_info, {"epoch", "step"}])`, and
fires handlers -- objects with `.run(state, event)` -- on six events.  `opt.py:96-140` wires training with exactly these
pieces: train engine {STEP_COMPLETED: ScalarMovingAverage; EPOCH_COMPLETED: TrackLr, PeriodicSaver, TriggerEngine("valid"),
ScheduleLr}, valid engine {STEP_COMPLETED: AccumulateRawOutput; EPOCH_COMPLETED: ProcessAccumulatedRawOutput}.

This module provides the same surface -- event names, `State` fields, `add_event_handler`, `run(nr_epoch, shared_state,
chained)`, the handler protocol -- so the reference's own callback objects (logging, visualisation) attach unchanged, and
the data-path callbacks listed above so `hover_net_amd.train.run_phases` is the reference's wiring on the HIP step functions.
`VisualizeOutput` (callbacks/base.py:220-232) draws the epoch's training picture, on the device when the step kept its samples there.
Not rebuilt (host-only glue): tqdm progress bars, LoggingEpochOutput / LoggingGradient (tensorboard + json), ConditionalSaver."""
from enum import Enum

import torch


class Events(Enum):
    EPOCH_STARTED = "epoch_started"
    EPOCH_COMPLETED = "epoch_completed"
    STEP_STARTED = "step_started"
    STEP_COMPLETED = "step_completed"
    STARTED = "started"
    COMPLETED = "completed"
    EXCEPTION_RAISED = "exception_raised"


class State:
    """Shared between the handlers of one engine (engine.py:17-72: same field names)."""

    def __init__(self):
        self.logging = None
        self.log_dir = None
        self.log_info = None
        self.curr_epoch_step = 0
        self.curr_global_step = 0
        self.curr_epoch = 0
        self.tracked_step_output = {"scalar": {}, "image": {}}
        self.epoch_accumulated_output = {}
        self.run_accumulated_output = []
        self.step_output = None
        self.global_state = None
        self.pertain_n_epoch_output = 1

    def reset_variable(self):
        self.tracked_step_output = {k: {} for k in self.tracked_step_output}
        if self.curr_epoch % self.pertain_n_epoch_output == 0:
            self.run_accumulated_output = []
        self.epoch_accumulated_output = {}
        self.step_output = None


class RunEngine:
    def __init__(self, engine_name=None, dataloader=None, run_step=None, run_info=None, log_info=None):
        self.engine_name, self.run_step, self.dataloader = engine_name, run_step, dataloader
        self.state = State()
        self.state.attached_engine_name = engine_name
        self.state.run_info = run_info
        self.state.log_info = log_info
        self.state.batch_size = getattr(dataloader, "batch_size", None)
        self.state.dataloader = dataloader          # not a reference field: DeviceValidStats reads the loader's n_samples from it
        self.event_handler_dict = {event: [] for event in Events}
        self.terminate = False

    def add_event_handler(self, event_name, handler):
        self.event_handler_dict[event_name].append(handler)

    def _trigger(self, event):
        for handler in self.event_handler_dict[event]:
            handler.run(self.state, event)

    def run(self, nr_epoch=1, shared_state=None, chained=False):
        if chained:                              # a triggered engine (validation) starts over every time
            self.state.curr_epoch = 0
        self.state.global_state = shared_state
        while self.state.curr_epoch < nr_epoch:
            self.state.reset_variable()
            self._trigger(Events.EPOCH_STARTED)
            for data_batch in self.dataloader:
                self._trigger(Events.STEP_STARTED)
                info = [self.state.run_info, {"epoch": self.state.curr_epoch, "step": self.state.curr_global_step}]
                self.state.step_output = self.run_step(data_batch, info)
                self._trigger(Events.STEP_COMPLETED)
                self.state.curr_global_step += 1
                self.state.curr_epoch_step += 1
            self.state.curr_epoch += 1
            self._trigger(Events.EPOCH_COMPLETED)
            self.state.run_accumulated_output.append(self.state.epoch_accumulated_output)


# ---- the data-path callbacks of run_utils/callbacks/base.py ----------------------------------------------------------------------
class BaseCallbacks:
    def __init__(self):
        self.engine_trigger = False

    def reset(self):
        pass

    def run(self, state, event):
        pass


class TrackLr(BaseCallbacks):
    def run(self, state, event):
        for net_name, net_info in state.run_info.items():
            state.tracked_step_output["scalar"]["lr-%s" % net_name] = net_info["optimizer"].param_groups[0]["lr"]


class ScheduleLr(BaseCallbacks):
    def run(self, state, event):
        for net_info in state.run_info.values():
            net_info["lr_scheduler"].step()


class TriggerEngine(BaseCallbacks):
    def __init__(self, triggered_engine_name, nr_epoch=1):
        super().__init__()
        self.engine_trigger = True
        self.triggered_engine_name = triggered_engine_name
        self.triggered_engine = None            # bound by the wiring code (run_train.py:250-254)
        self.nr_epoch = nr_epoch

    def run(self, state, event):
        self.triggered_engine.run(chained=True, nr_epoch=self.nr_epoch, shared_state=state)


class ScalarMovingAverage(BaseCallbacks):
    def __init__(self, alpha=0.95):
        super().__init__()
        self.alpha = alpha
        self.tracking_dict = {}

    def run(self, state, event):
        for key, value in state.step_output["EMA"].items():
            old = self.tracking_dict.get(key)
            self.tracking_dict[key] = value if old is None else old * self.alpha + (1.0 - self.alpha) * value
        state.tracked_step_output["scalar"] = self.tracking_dict


class AccumulateRawOutput(BaseCallbacks):
    def run(self, state, event):
        acc = state.epoch_accumulated_output
        for key, value in state.step_output["raw"].items():
            acc.setdefault(key, []).extend(list(value))


class ProcessAccumulatedRawOutput(BaseCallbacks):
    def __init__(self, proc_func, per_n_epoch=1):
        super().__init__()
        self.per_n_epoch = per_n_epoch
        self.proc_func = proc_func

    def run(self, state, event):
        state.tracked_step_output = self.proc_func(state.epoch_accumulated_output)


class VisualizeOutput(BaseCallbacks):
    """callbacks/base.py:220-232, EPOCH_COMPLETED of the train engine: the picture of the epoch's last step,
    `state.tracked_step_output["image"]["output"] = proc_func(state.step_output["raw"])` (`proc_func`: `run_desc.viz_step_output`,
    or a lambda that adds nr_types).  When "raw" holds device tensors (`train_step` with `extra_info["viz"] == "device"`) it is
    `device_func` that draws, on the device, and the finished strip is what comes to the host.  `per_n_epoch` is kept and, as in
    the reference, not consulted.  An epoch without a step draws nothing."""

    def __init__(self, proc_func, per_n_epoch=1, device_func=None):
        super().__init__()
        self.per_n_epoch = per_n_epoch
        self.proc_func = proc_func
        self.device_func = device_func

    def run(self, state, event):
        if state.step_output is None:
            return
        raw = state.step_output["raw"]
        img = raw.get("img") if hasattr(raw, "get") else None
        if torch.is_tensor(img) and img.is_cuda:
            from . import run_desc

            strip = (self.device_func or run_desc.viz_step_output_device)(raw)
            state.tracked_step_output["image"]["output"] = strip.cpu().numpy()
        else:
            state.tracked_step_output["image"]["output"] = self.proc_func(raw)


class DeviceValidStats(BaseCallbacks):
    """EPOCH_COMPLETED of a valid engine whose step is `run_desc.valid_step_stats`: in place of AccumulateRawOutput +
    ProcessAccumulatedRawOutput.  `stats` (a `valid_stats.ValidStats`) is merged over the ranks -- a collective: every rank's valid
    engine must reach this point once per epoch --, read once and cleared for the next epoch.

    `viz_samples > 0` adds the epoch's picture (`tracked_step_output["image"]["output"]`, the reference draws eight patches, with
    replacement): the handler must then ALSO be registered for EPOCH_STARTED, where it plans that epoch's samples
    (`ValidStats.plan_viz`) from `n_samples` of the engine's loader (`state.dataloader`; `augment.DevicePatchLoader` has it), drawn from
    `numpy.random.default_rng([seed, k])` for the k-th plan.  A loader without `n_samples` gets no picture -- how many samples an epoch
    holds cannot be known before it ran.  Pictures come from rank 0's shard only; the other ranks plan nothing."""

    def __init__(self, stats, viz_samples=0, seed=0):
        super().__init__()
        self.stats = stats
        self.viz_samples, self.seed, self._plans = int(viz_samples), int(seed), 0

    def plan(self, loader):
        """Plan the coming epoch's picture (EPOCH_STARTED does this); returns the planned indices or None."""
        n = getattr(loader, "n_samples", None)
        if self.viz_samples <= 0 or not n or _rank() != 0:
            return None
        import numpy as np

        idx = np.random.default_rng([self.seed, self._plans]).integers(0, int(n), size=self.viz_samples)
        self._plans += 1
        self.stats.plan_viz(idx, getattr(loader, "input_shape", None))
        return idx

    def run(self, state, event):
        if event == Events.EPOCH_STARTED:
            self.plan(getattr(state, "dataloader", None))
            return
        self.stats.merge_ranks()
        state.tracked_step_output = self.stats.track()
        self.stats.reset()


def _rank():
    import torch.distributed as dist

    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class PeriodicSaver(BaseCallbacks):
    """`{net_name}_epoch={n}.tar` = {key: value.state_dict()} for every entry of the net's run_info except extra_info
    (desc, optimizer, lr_scheduler), written by the process whose `state.logging` is set (rank 0)."""

    def __init__(self, per_n_epoch=1, per_n_step=None):
        super().__init__()
        self.per_n_epoch = per_n_epoch
        self.per_n_step = per_n_step

    def run(self, state, event):
        if not state.logging or state.curr_epoch % self.per_n_epoch != 0:
            return
        for net_name, net_info in state.run_info.items():
            ckpt = {}
            for key, value in net_info.items():
                if key == "extra_info":
                    continue
                sd = value.state_dict()
                if key == "desc":
                    sd = {k: v.detach().cpu().contiguous() for k, v in sd.items()}
                ckpt[key] = sd
            torch.save(ckpt, "%s/%s_epoch=%d.tar" % (state.log_dir, net_name, state.curr_epoch))
