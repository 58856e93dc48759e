"""AdamStateOptimizer: the per-parameter state (``step``, ``exp_avg``, ``exp_avg_sq``) and the device step counters that
FusedAdamW and FusedLAMB share.  The state-dict layout is torch.optim.AdamW's."""
from __future__ import annotations

import torch

from ..ops import multi_tensor as mt
from ._fused import FusedOptimizer
from ._grads import grad_of


class AdamStateOptimizer(FusedOptimizer):
    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._dsteps: dict = {}

    def _counters(self, present):
        """Device step counters for this step's parameters (those with a gradient), as [(counter, params)].

        torch counts steps per parameter.  Parameters whose step histories are identical share ONE device counter
        (one ``step_inc`` launch, one step launch); a counter whose parameters did not all get a gradient this
        step is split (the ones stepping get a clone), so a parameter that skips steps -- an unused branch, a late
        unfreeze -- keeps its own count and bias correction.  Parameters without a counter (new state, or a host
        step loaded from a checkpoint) are grouped by their step value.  ``_dsteps``: id(counter) -> (counter,
        set of ids of the parameters sharing it)."""
        members = self._dsteps
        shared, fresh = {}, {}
        for p in present:
            c = self._init_state(p)["step"]
            ent = members.get(id(c))
            if ent is not None and ent[0] is c:
                shared.setdefault(id(c), []).append(p)
            else:
                fresh.setdefault((float(c), p.device), []).append(p)
        out = []
        for (v, dev), ps in fresh.items():
            c = torch.full((), v, dtype=torch.float32, device=dev)
            for p in ps:
                old = self.state[p]["step"]
                ent = members.get(id(old))
                if ent is not None and ent[0] is old:
                    ent[1].discard(id(p))
                    if not ent[1]:
                        del members[id(old)]
                self.state[p]["step"] = c
            members[id(c)] = (c, {id(p) for p in ps})
            out.append((c, ps))
        for cid, ps in shared.items():
            c, mem = members[cid]
            if len(ps) != len(mem):
                ids = {id(p) for p in ps}
                mem -= ids
                c = c.clone()
                members[id(c)] = (c, ids)
                for p in ps:
                    self.state[p]["step"] = c
            out.append((c, ps))
        return out

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dsteps.clear()     # device step counters are rebuilt from the loaded per-parameter steps

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format, dtype=torch.float32)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format, dtype=torch.float32)
            p._pdt_opt_state = True
        return st

    def _count_step(self, group, found_inf):
        """Advance the step count of the group's parameters that have a gradient and bucket them for the launches:
        -> (buckets {(grad dtype, counter key, device): [params]}, counters {counter key: device counter}), or None
        when a host ``found_inf`` flag skips the step.  A bucket whose key is not in ``counters`` counts on the host:
        its step is ``-key``."""
        buckets = {}
        cap = bool(group.get("capturable", False))
        # An overflowed fp16 step (found_inf != 0) must leave params, moments AND the step count alone:
        # torch.amp.GradScaler skips optimizer.step() entirely.  With a device flag the count lives on the
        # device and advances conditionally (pdt_step_inc), so no host sync is needed; once a parameter has a
        # device count it keeps it (mixing the two counters would double-count).
        # GPU parameters always count on the device: one step_inc launch per counter instead of a host tensor
        # add + .item() per parameter (161 of them for ResNet-50: ~1 ms of host time per step, a GPU-idle gap
        # in front of the AdamW launch -- profiles/r3_s4h_resnet50-ddp_kernel_table.txt)
        on_gpu = bool(group["params"]) and group["params"][0].device.type == "cuda"
        dev_step = cap or on_gpu or (found_inf is not None and found_inf.device.type == "cuda") or any(
            id(self.state[p].get("step")) in self._dsteps for p in group["params"] if p in self.state)
        if found_inf is not None and found_inf.device.type != "cuda" and int(found_inf.reshape(-1)[0]) != 0:
            return None
        present = self._present(group)
        counters = {}
        if dev_step:
            for c, ps in self._counters(present):
                mt.step_inc_(c, found_inf)    # one device increment per counter (graph-capturable)
                counters[id(c)] = c
                for p in ps:
                    buckets.setdefault((grad_of(p).dtype, id(c), p.device), []).append(p)
        else:
            for p in present:
                st = self._init_state(p)
                st["step"] += 1
                buckets.setdefault((grad_of(p).dtype, -int(st["step"].item()), p.device), []).append(p)
        return buckets, counters
