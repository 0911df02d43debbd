"""One CGC (customized gate control) level of PLE, the reference module's constructor, attribute names, forward and return
value (tzrec/modules/extraction_net.py:20-139): `expert_num_per_task` expert MLPs per task over that task's input, `share_num`
shared ones over the shared input; task gate t = Linear + softmax over [its own experts | the shared ones] of its input, the
shared gate (absent on the last level) over [all task experts in task order | the shared ones] of the shared input.  The
gate-and-mix step of the whole level is one launch per direction (gate_ops.cgc_mix, csrc/gate_mix.hip)."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from .dlrm import MLP, OutputLinear

FUSED_CGC_MIX = True  # A/B switch: False = the reference's stack / softmax / batched-matmul form per gate


class ExtractionNet(nn.Module):
    def __init__(self, in_extraction_networks: List[int], in_shared_expert: int, network_name: str, share_num: int,
                 expert_num_per_task: int, share_expert_net: Dict[str, object], task_expert_net: Dict[str, object],
                 final_flag: bool = False) -> None:
        super().__init__()
        self.name = network_name
        self._final_flag = final_flag
        self._output_dims: List[int] = []
        self._shared_layers = nn.ModuleList([MLP(in_shared_expert, **share_expert_net) for _ in range(share_num)])
        n_task = len(in_extraction_networks)
        # (OutputLinear: nn.Linear's parameters; <= 8 units the one-pass kernels, more nn.Linear's own GEMM)
        self._shared_gate = None if final_flag else OutputLinear(in_shared_expert, n_task * expert_num_per_task + share_num)
        self._task_layers = nn.ModuleList()
        self._task_gates = nn.ModuleList()
        for d in in_extraction_networks:
            self._task_layers.append(nn.ModuleList([MLP(d, **task_expert_net) for _ in range(expert_num_per_task)]))
            self._task_gates.append(OutputLinear(d, expert_num_per_task + share_num))
            self._output_dims.append(task_expert_net["hidden_units"][-1])
        self._output_dims.append(share_expert_net["hidden_units"][-1])
        # member lists over experts = [task 0's | task 1's | ... | shared], each in the order of its gate's logit columns
        P, first_shared = expert_num_per_task, n_task * expert_num_per_task
        shared = list(range(first_shared, first_shared + share_num))
        self._sels = [list(range(t * P, (t + 1) * P)) + shared for t in range(n_task)]
        if not final_flag:
            self._sels.append(list(range(first_shared)) + shared)

    def output_dim(self) -> List[int]:
        """width of every task output, then of the shared output"""
        return self._output_dims

    def forward(self, extraction_network_fea: List[torch.Tensor], shared_expert_fea: torch.Tensor) -> Tuple[List[torch.Tensor], Optional[torch.Tensor]]:
        experts: List[torch.Tensor] = []
        for x, layers in zip(extraction_network_fea, self._task_layers):
            experts.extend(layer(x) for layer in layers)
        experts.extend(layer(shared_expert_fea) for layer in self._shared_layers)
        logits = [gate(x) for x, gate in zip(extraction_network_fea, self._task_gates)]
        if self._shared_gate is not None:
            logits.append(self._shared_gate(shared_expert_fea))
        outs = None
        if FUSED_CGC_MIX and shared_expert_fea.dim() == 2 and (shared_expert_fea.is_cuda or _lib.emulated()):
            from .gate_ops import cgc_mix, cgc_mix_ok

            if cgc_mix_ok(logits, experts, self._sels):  # every gate of the level in one launch per direction, nothing stacked
                outs = cgc_mix(logits, experts, self._sels)
        if outs is None:  # the reference's literal form
            outs = [torch.matmul(torch.softmax(lg, dim=1).unsqueeze(1), torch.stack([experts[e] for e in sel], dim=1)).squeeze(1)
                    for lg, sel in zip(logits, self._sels)]
        n_task = len(self._task_layers)
        return outs[:n_task], (outs[n_task] if self._shared_gate is not None else None)
