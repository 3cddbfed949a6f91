"""The range guard of the f16x2 inference paths, shared by the engines (cpd_amd/engine.py, anchor_engine.py) and the fused module path
(spconv/pytorch/conv.py, models.CenterPoint._run_modules).

Split-fp16 arithmetic is exact only below 2^15. An OPTIMISTIC step runs the unscaled kernels, whose epilogues record max |out| into the
absmax blocks of a `BlockPool`; the pool's verdict rides along with the step's one count read-back, and a step that reached 2^15 is run
again GUARDED -- every layer pre-scaling its input by its block's power of two: exact at any magnitude. `RangeGuard` then keeps its owner
guarded for `sticky` steps, so that a model which habitually leaves the range pays the guarded kernels' ~3 % and not a second pass per step."""
import warnings

import torch

from . import ops

OPTIMISTIC_BITS = 0x47000000      # bits of 32768.0f: an optimistic step at or above it is run again guarded
GUARDED_BITS = 0x46800000         # bits of 16384.0f: a guarded step at or above it extends the guarded stay (hysteresis)


class BlockPool:
    """the absmax blocks of one step or pass, one per conv launch, handed out in launch order"""

    def __init__(self, exhausted):
        self.exhausted = exhausted            # the owner's error text, with one %d for the pool's size
        self.blocks, self.next, self._key = None, 0, None

    def reset(self, n, device):
        """all blocks zero and the cursor at the first; (re)allocated on first use and when the size or the device changes"""
        key = (int(n), torch.device(device))
        if key != self._key:
            self.blocks, self._key = ops.absmax_blocks(*key), key
        else:
            self.blocks.zero_()
        self.next = 0

    def new_block(self):
        i = self.next
        if i >= self.blocks.shape[0]:
            raise RuntimeError(self.exhausted % self.blocks.shape[0])
        self.next = i + 1
        return self.blocks[i]

    def flag(self, threshold_bits):
        """device int32 [1]: 1 when some recorded |activation| is >= the threshold (the bit patterns of NaN and inf are larger still)"""
        return (self.blocks.max() >= threshold_bits).to(torch.int32).view(1)


class RangeGuard:
    """the hysteresis of the guard and its counters: `scaled` = the current step runs guarded, `left` = guarded steps still to come,
    `reruns` = steps that were run twice, `guarded_steps` = steps that ended on the guarded kernels"""

    def __init__(self, sticky, owner="engine"):
        self.sticky, self.owner = sticky, owner      # owner: who the warning says stays guarded ("engine" / "model")
        self.left = self.reruns = self.guarded_steps = 0
        self.scaled = self.high = False

    def begin_step(self):
        self.scaled = self.left > 0

    def verdict(self, bit):
        """once per pass, with the pool's flag as read back: must the step be run again? A guarded pass is exact whatever the range:
        never; its flag (>= 2^14) only keeps the owner guarded (end_step)."""
        if self.scaled:
            self.high = bool(bit)
            return False
        return bool(bit)

    def trip(self):
        """an optimistic pass left the range: the step is run again guarded, and the owner stays guarded"""
        if self.reruns == 0:
            warnings.warn("cpd_amd: an activation reached 2^15 -- step re-run with the range-guarded f16x2 kernels; the %s stays "
                          "guarded for the next %d steps" % (self.owner, self.sticky), stacklevel=2)
        self.scaled = True
        self.reruns += 1
        self.left = self.sticky + 1

    def end_step(self):
        if self.scaled:
            self.guarded_steps += 1
            self.left = self.sticky if self.high else self.left - 1
        self.scaled = self.high = False
