"""The personalization modules of PEPNet, the reference's constructors, attribute names, parameter order, state-dict keys and
`detach()` placement (tzrec/modules/personalized_net.py): `GateNU` = gamma * sigmoid(Linear(relu(Linear(x)))), `EPNet` scales the
main embedding by a gate over [domain | main.detach()], `PPNet` runs per task a stack of Linear -> activation -> times a gate
over [uia | main.detach()] -> dropout.  Everything behind the three GEMMs of a (task, layer) -- two bias adds, the ReLU, the
sigmoid, the scale by gamma and the multiply, and in the backward the two bias gradients -- is one launch per PPNet level for
all tasks, and one for EPNet (gate_ops.gate_scale, csrc/gate_scale.hip)."""
from __future__ import annotations

from typing import List, Optional, Union

import torch
from torch import nn

from . import _lib
from .dlrm import _activation

FUSED_GATE_SCALE = True  # A/B switch: False = the reference's literal form, op by op


def _fusable(x: torch.Tensor) -> bool:
    return bool(FUSED_GATE_SCALE and x.dim() == 2 and (x.is_cuda or _lib.emulated()))


class GateNU(nn.Module):
    def __init__(self, input_dim: int, hidden_dim: int, output_dim: int, gamma: float = 2.0) -> None:
        super().__init__()
        self._gamma = gamma
        self._output_dim = output_dim
        self.dense_layers = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, output_dim), nn.Sigmoid())

    def output_dim(self) -> int:
        return self._output_dim

    def pre_sigmoid(self, x: torch.Tensor) -> torch.Tensor:
        """relu(Linear(x)) times the second layer's weight, WITHOUT its bias: the `g` of gate_ops.gate_scale"""
        first, second = self.dense_layers[0], self.dense_layers[2]
        return nn.functional.linear(torch.relu(first(x)), second.weight)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._gamma * self.dense_layers(x)


class EPNet(nn.Module):
    def __init__(self, main_dim: int, domain_dim: int, hidden_dim: int, gamma: float = 2.0) -> None:
        super().__init__()
        self._domain_dim = domain_dim
        self._main_dim = main_dim
        self.gate_nu = GateNU(input_dim=domain_dim + main_dim, hidden_dim=hidden_dim, output_dim=main_dim, gamma=gamma)

    def output_dim(self) -> int:
        return self.gate_nu.output_dim()

    def forward(self, main_emb: torch.Tensor, domain_emb: torch.Tensor) -> torch.Tensor:
        gate_input = torch.cat([domain_emb, main_emb.detach()], dim=-1)
        if _fusable(main_emb) and main_emb.dtype == torch.float32 and main_emb.shape[0] > 0:
            from .gate_ops import gate_scale, gate_scale_ok

            z, g = _lib.rows16(main_emb), self.gate_nu.pre_sigmoid(gate_input)
            bg = [self.gate_nu.dense_layers[2].bias]
            if gate_scale_ok([z], [g], [None], bg):  # one launch: identity, no bias on the main embedding
                return gate_scale([z], [None], [g], bg, self.gate_nu._gamma, relu=False)[0]
        return self.gate_nu(gate_input) * main_emb  # the reference's literal form


class PPNet(nn.Module):
    def __init__(self, main_feature: int, uia_feature: int, num_task: int, hidden_units: List[int], activation: Optional[str] = "nn.ReLU",
                 dropout_ratio: Optional[Union[List[float], float]] = None, gamma: float = 2.0) -> None:
        super().__init__()
        self.main_feature = main_feature
        self.uia_feature = uia_feature
        self.num_task = num_task
        self.hidden_units = hidden_units
        self.len_hidden = len(hidden_units)
        self.linears = nn.ModuleList()
        self.activations = nn.ModuleList()
        self.dropout_ratios = nn.ModuleList()
        self.gate_nus = nn.ModuleList()
        if dropout_ratio is None:
            dropout_ratio = [0.0] * len(hidden_units)
        elif isinstance(dropout_ratio, list):
            if len(dropout_ratio) == 0:
                dropout_ratio = [0.0] * len(hidden_units)
            elif len(dropout_ratio) == 1:
                dropout_ratio = dropout_ratio * len(hidden_units)
            elif len(dropout_ratio) != len(hidden_units):
                raise ValueError(f"length of dropout_ratio and hidden_units must be same, but got {len(dropout_ratio)} vs {len(hidden_units)}")
        else:
            dropout_ratio = [dropout_ratio] * len(hidden_units)
        self._relu = activation == "nn.ReLU"
        self._gamma = gamma
        for _ in range(num_task):
            output = main_feature
            for i, hidden_unit in enumerate(hidden_units):
                self.linears.append(nn.Linear(output, hidden_unit))
                act = _activation(activation)
                self.activations.append(act if act is not None else nn.Identity())
                self.dropout_ratios.append(nn.Dropout(dropout_ratio[i]))
                self.gate_nus.append(GateNU(input_dim=main_feature + uia_feature, hidden_dim=hidden_unit, output_dim=hidden_unit, gamma=gamma))
                output = hidden_unit

    def output_dim(self) -> List[int]:
        return [self.hidden_units[-1]] * self.num_task

    def task_output_dim(self) -> int:
        return self.hidden_units[-1]

    def forward(self, main_emb: torch.Tensor, uia_emb: torch.Tensor) -> List[torch.Tensor]:
        gate_input = torch.cat([uia_emb, main_emb.detach()], dim=-1)  # (the same tensor for every task: built once)
        fused = self._relu and _fusable(main_emb)
        inputs = [main_emb] * self.num_task
        for j in range(self.len_hidden):
            idx = [i * self.len_hidden + j for i in range(self.num_task)]
            outs = None
            if fused:
                from .gate_ops import gate_scale, gate_scale_ok

                zs = [nn.functional.linear(x, self.linears[k].weight) for x, k in zip(inputs, idx)]  # the GEMMs without bias
                gs = [self.gate_nus[k].pre_sigmoid(gate_input) for k in idx]
                bzs = [self.linears[k].bias for k in idx]
                bgs = [self.gate_nus[k].dense_layers[2].bias for k in idx]
                if gate_scale_ok(zs, gs, bzs, bgs):  # every task of the level in one launch per direction
                    outs = gate_scale(zs, bzs, gs, bgs, self._gamma, relu=True)
            if outs is None:  # the reference's literal form
                outs = [self.activations[k](self.linears[k](x)) * self.gate_nus[k](gate_input) for x, k in zip(inputs, idx)]
            inputs = [self.dropout_ratios[k](o) for o, k in zip(outs, idx)]
        return inputs
