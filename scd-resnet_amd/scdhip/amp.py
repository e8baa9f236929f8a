"""Dynamic loss scaling for the fp16 compute mode (the rule of torch.amp.GradScaler on the flat optimizers).

The scale S stays a host value, ``ops.LossScale.f16``: the heads backward multiplies by it and every parameter-gradient
reduction multiplies by 1/S, so ``FlatParams.grad`` holds unscaled fp32 gradients.  What an overflow in the fp16
backward leaves there is an inf or a NaN.  With a ``DynamicLossScale`` attached, ``optimizer.step()`` queues
``scd_grad_guard`` over the flat gradient right before the optimizer kernel and hands its verdict to that kernel as
the skip word, so an overflowed step changes nothing on the device (parameters, moments / momentum buffer, step
counter).  The host learns the verdict later, from a pinned ring it never waits on unless the ring is full:

    found:  S = max(S * backoff_factor, min_scale), tracker = 0
    clean:  tracker += 1; at growth_interval: S = min(S * growth_factor, max_scale), tracker = 0

One addition covers the lag between a step and its verdict: a found verdict of a step that ran at a scale other than
the current one resets the tracker but does not back off again -- that scale has been left already.  Two overflowing
steps issued before the host hears of the first halve S once.  Call ``update()`` after ``step()`` (the step is tagged
with the scale in force when it is issued, which is the scale its backward ran at).

Every factor and bound is a power of two, so 1/S stays an exact unscale.  A data-parallel run checks the all-reduced
gradient, which every rank holds alike, so every rank reaches the same verdict without exchanging anything (no
multi-rank run has been made: one GPU here).
"""
import collections
import math

import torch

from . import ops


def is_pow2(x):
    """x is a positive, finite power of two (2**k, k any integer)."""
    x = float(x)
    return x > 0.0 and math.isfinite(x) and math.frexp(x)[0] == 0.5


def scale_rule(scale, tracker, found, ran_at, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
               min_scale=1.0, max_scale=2.0 ** 24):
    """One step's verdict applied to (scale, tracker): the pure host rule ``DynamicLossScale.update`` uses.
    found: the step's gradient held a non-finite element; ran_at: the scale that step ran at."""
    if found:
        if ran_at == scale:
            scale = max(scale * backoff_factor, min_scale)
        return scale, 0
    tracker += 1
    if tracker >= growth_interval:
        return min(scale * growth_factor, max_scale), 0
    return scale, tracker


_Slot = collections.namedtuple("_Slot", "index event ran_at")


class DynamicLossScale:
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
                 min_scale=1.0, max_scale=2.0 ** 24, depth=8):
        for name, v in (("init_scale", init_scale), ("growth_factor", growth_factor),
                        ("backoff_factor", backoff_factor), ("min_scale", min_scale), ("max_scale", max_scale)):
            if not is_pow2(v):
                raise ValueError("DynamicLossScale: %s = %r is not a power of two (1/scale must stay an exact "
                                 "unscale)" % (name, v))
        if growth_factor <= 1.0 or backoff_factor >= 1.0:
            raise ValueError("DynamicLossScale: growth_factor must be above 1 and backoff_factor below 1")
        if int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError("DynamicLossScale: growth_interval = %r must be an integer >= 1" % (growth_interval,))
        if min_scale > init_scale or init_scale > max_scale:
            raise ValueError("DynamicLossScale: need min_scale <= init_scale <= max_scale, got %r, %r, %r"
                             % (min_scale, init_scale, max_scale))
        if int(depth) != depth or depth < 1:
            raise ValueError("DynamicLossScale: depth = %r must be an integer >= 1" % (depth,))
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.min_scale = float(min_scale)
        self.max_scale = float(max_scale)
        self.depth = int(depth)
        self._scale = float(init_scale)
        self._tracker = 0
        self.skipped = 0
        self.steps = 0
        self.grad_norm = None
        self.last_nonfinite = 0         # non-finite count of the last processed step
        self.on_change = None           # callable(old_scale, new_scale, nonfinite_count), called by update()
        self._optimizer = None
        self._static = None
        self._pending = collections.deque()
        self._free = list(range(self.depth))
        self._dev = None                # device: {skip word, non-finite count, sumsq bits}
        self._ws = None
        self._host = None               # pinned (depth, 3) ring
        self._events = None

    # ---- host state
    @property
    def scale(self):
        return self._scale

    def _set_scale(self, S):
        self._scale = float(S)
        if self._optimizer is not None:
            ops.set_loss_scale(self._scale)

    def attach(self, optimizer):
        if self._optimizer is not None:
            raise RuntimeError("DynamicLossScale: already attached to an optimizer")
        if not hasattr(optimizer, "_attach_scaler"):
            raise TypeError("DynamicLossScale.attach: needs a FlatAdam or FlatSGD, got %s" % type(optimizer).__name__)
        optimizer._attach_scaler(self)
        self._optimizer = optimizer
        self._static = ops.set_loss_scale(self._scale)
        return self

    def detach(self):
        """Apply what is outstanding, leave the optimizer and restore the static scale in force at attach."""
        if self._optimizer is None:
            return
        self.update(block=True)
        self._optimizer._attach_scaler(None)
        self._optimizer = None
        ops.set_loss_scale(self._static)
        self._static = None

    # ---- the step side (called by the optimizer's step())
    def _buffers(self, dev):
        if self._dev is None:
            self._dev = torch.zeros(3, dtype=torch.int64, device=dev)
            self._ws = torch.zeros(ops.grad_guard_workspace(0), dtype=torch.uint8, device=dev)
            self._host = torch.zeros(self.depth, 3, dtype=torch.int64).pin_memory()
            self._events = [torch.cuda.Event() for _ in range(self.depth)]

    def guard(self, grad, also=None):
        """Queue the guard over the flat gradient on the current stream and the copy of its verdict into a ring slot;
        returns the device skip word for the optimizer kernel."""
        if ops.capturing():
            raise RuntimeError("DynamicLossScale: a captured step graph bakes the scale into its launches; dynamic "
                               "loss scaling runs eager steps only")
        self._buffers(grad.device)
        ran_at = self._scale                    # the scale this step's backward ran at: read before the ring moves it
        if not self._free:
            self._process(self._pending.popleft(), block=True)      # ring full: bounds the lag to `depth` steps
        ops.grad_guard(grad, self._ws, self._dev[:2], self._dev[2:], also=also)
        i = self._free.pop()
        self._host[i].copy_(self._dev, non_blocking=True)
        self._events[i].record()
        self._pending.append(_Slot(i, self._events[i], ran_at))
        return self._dev

    # ---- the host side
    def _process(self, slot, block):
        if block:
            slot.event.synchronize()
        row = self._host[slot.index]
        skip, count = int(row[0]), int(row[1])
        sumsq = float(row[2:3].view(torch.float64)[0])
        self._free.append(slot.index)
        self.steps += 1
        self.grad_norm = math.sqrt(sumsq)
        self.last_nonfinite = count
        if skip:
            # nothing moved on the device, its step counter included: take the step back off the host mirror
            self.skipped += 1
            self._optimizer._step -= 1
        if skip and not count:
            return                          # skipped for the peer-SyncBN error word alone: no word on the scale
        old = self._scale
        S, self._tracker = scale_rule(old, self._tracker, count != 0, slot.ran_at, self.growth_factor,
                                      self.backoff_factor, self.growth_interval, self.min_scale, self.max_scale)
        if S != old:
            self._set_scale(S)
            if self.on_change is not None:
                self.on_change(old, S, count)

    def update(self, block=False):
        """Apply the verdicts of finished steps, oldest first; block=True waits for every outstanding one."""
        while self._pending:
            if not block and not self._pending[0].event.query():
                break
            self._process(self._pending.popleft(), block)
        return self._scale

    # ---- checkpoints
    def state_dict(self):
        return {"scale": self._scale, "tracker": self._tracker, "skipped": self.skipped, "steps": self.steps}

    def load_state_dict(self, sd):
        if not is_pow2(sd["scale"]) or not self.min_scale <= sd["scale"] <= self.max_scale:
            raise ValueError("DynamicLossScale.load_state_dict: scale %r is not a power of two within [%r, %r]"
                             % (sd["scale"], self.min_scale, self.max_scale))
        self.update(block=True)
        self._set_scale(sd["scale"])
        self._tracker = int(sd["tracker"])
        self.skipped = int(sd["skipped"])
        self.steps = int(sd["steps"])
