"""Dense crowds (21..127 humans) for the SARL tests: the seeded roots both test files use, their float64 search (tests/sarl_cpu.py)
and the float32 restatement of the same scenes -- upstream's own arithmetic, whose distance from float64 on a case's own scenes is
one of the two numbers a case's bound is the larger of (the other: the bound of the small crowds, sarl_cpu.value_bound /
attention_bound).  Rows are built once per (H, input_dim, root) and shared by every test that needs them."""
import functools

import numpy as np
import torch

from tests import sarl_cpu as cpu

DENSE_H = [21, 33, 50, 127]
INPUT_DIMS = [13, 29, 45, 61]
ROOTS = 2          # 162 scenes: ten tiles of sixteen and one of two


def kinematics_of(H, input_dim):
    return "unicycle" if (H + input_dim) % 2 else "holonomic"


@functools.lru_cache(maxsize=None)
def roots(H, input_dim):
    """(robot (ROOTS,9), humans (ROOTS,H,5)) float64 of one crowd size and row width."""
    return cpu.scenes(7000 + H, ROOTS, H, kinematics_of(H, input_dim))


@functools.lru_cache(maxsize=None)
def root_rows(H, input_dim, b):
    robot, humans = roots(H, input_dim)
    rows, reward, _ = cpu.search_rows(robot[b], humans[b], kinematics_of(H, input_dim), cpu.om_of(input_dim))
    return rows, reward


def case(H, input_dim, with_global_state, weights):
    """Per root: rows (A,H,D) float32, the float64 value / attention / action values / decision, and the float32 restatement's
    largest distance from them on the action values (dev_value) and on the attention weights of every action (dev_attention)."""
    sd = cpu.weight_set(weights, input_dim, with_global_state)
    robot, _ = roots(H, input_dim)
    out = []
    for b in range(ROOTS):
        rows, reward = root_rows(H, input_dim, b)
        v64, a64 = cpu.value_network(rows, sd, with_global_state, torch.float64)
        v32, a32 = cpu.value_network(rows, sd, with_global_state, torch.float32)
        av64, best = cpu.decide(reward, v64.numpy(), robot[b, 7])
        av32, best32 = cpu.decide(reward, v32.double().numpy(), robot[b, 7])
        out.append(dict(rows=rows, reward=reward, value=v64.numpy(), attention=a64.numpy(), action_values=av64, best=best,
                        best32=best32, dev_value=float(np.abs(av32 - av64).max()),
                        dev_attention=float(np.abs(a32.double().numpy() - a64.numpy()).max())))
    return out


def bounds(weights, roots_of_case):
    """(value bound, attention bound) of one case: the small crowds' bound, or four times the float32 restatement's own distance
    from float64 on this case's scenes where that is larger (sharp attention at 127 humans)."""
    dv = max(r["dev_value"] for r in roots_of_case)
    da = max(r["dev_attention"] for r in roots_of_case)
    return max(cpu.value_bound(weights), 4 * dv), max(cpu.attention_bound(weights), 4 * da)
