"""The plain torch restatement of MixtureOfExpertsLayer (MoE / MMoE) and of the two models built on it that the MoE tests
compare against (CPU, fp32 or fp64):
    out[b, g, k] = softmax_k(x2 W_g^T + b_g)[b, k] * cat_i(expert_i(x2))[b, k],   x2 = x.reshape(B, N*E)
tests/test_moe_host.py pins it to the reference's own outputs and gradients (tests/golden/moe.npz); the GPU tests use it at
sizes the fixture does not hold.  Also the shape lists shared by the generator (tests/golden/make_golden_moe.py) and the
tests."""
import torch
import torch.nn.functional as F

# (B, N, E, num_experts, Oi, G, expert_layer_sizes): layer cases of moe.npz
MOE_SHAPES = [(8, 4, 16, 4, 16, 1, [32, 16]), (5, 3, 8, 3, 5, 2, [16]), (16, 6, 16, 8, 16, 4, [16])]
# model cases of moe.npz: constructor arguments of the reference models (batch 16, dropout off)
MMOE_ARGS = dict(embed_size=8, num_fields=4, num_tasks=2, num_experts=3, expert_output_size=4, expert_layer_sizes=[16],
                 deep_layer_sizes=[8])
DEEPMOE_ARGS = dict(embed_size=8, num_fields=3, num_experts=3, moe_layer_sizes=[6, 4], deep_layer_sizes=[8])
MODEL_BATCH = 16
KINK_MARGIN = 1e-4          # the generator keeps every ReLU pre-activation at least this far from zero


def shape_tag(s):
    return "%d_%d_%d_x%d_%d_g%d_%s" % (s[0], s[1], s[2], s[3], s[4], s[5], "-".join(str(h) for h in s[6]))


def layer_kwargs(s):
    """constructor arguments of the layer for a case of MOE_SHAPES (expert_func is the caller's DNNLayer)"""
    B, N, E, X, Oi, G, hidden = s
    return dict(inputs_size=N * E, output_size=X * Oi, num_experts=X, num_gates=G, expert_inputs_size=N * E,
                expert_output_size=Oi, expert_layer_sizes=list(hidden))


def mlp(x, P, prefix, act=torch.relu, pre=None):
    """Linear_i + activation ... LinearOutput (multilayer_perceptron.py:53-61), parameters by state_dict key; ``pre``
    collects the pre-activations"""
    i = 0
    while f"{prefix}.model.Linear_{i}.weight" in P:
        x = F.linear(x, P[f"{prefix}.model.Linear_{i}.weight"], P[f"{prefix}.model.Linear_{i}.bias"])
        if pre is not None and act is not None:
            pre.append(x)
        x = act(x) if act is not None else x
        i += 1
    return F.linear(x, P[f"{prefix}.model.LinearOutput.weight"], P[f"{prefix}.model.LinearOutput.bias"])


def gate(logits, bias, experts):
    """(B, G*K) logits WITHOUT bias, (G*K) bias or None, (B, K) expert outputs -> (B, G, K): what the kernel computes"""
    B, K = experts.shape
    z = logits if bias is None else logits + bias
    return torch.softmax(z.reshape(B, -1, K), dim=2) * experts.unsqueeze(1)


def gate_backward(logits, bias, experts, gout):
    """glogits (B, G*K), gexperts (B, K) and the magnitude sum_k |p (t - sum p t)| (B, G) that a row of glogits sums over,
    written out: p = softmax(z), t = gout * e, glogits = p (t - sum_k p t), gexperts = sum_g gout p"""
    B, K = experts.shape
    z = logits if bias is None else logits + bias
    p = torch.softmax(z.reshape(B, -1, K), dim=2)
    t = gout * experts.unsqueeze(1)
    gl = p * (t - (p * t).sum(dim=2, keepdim=True))
    return gl.reshape(B, -1), (gout * p).sum(dim=1), gl.abs().sum(dim=2)


def moe_gate(x2, weight, bias, experts):
    """functional.moe_gate restated: stacked gate weights (G*K, D), biases (G*K) or None"""
    return gate(x2 @ weight.t(), bias, experts)


def moe_layer(x, P, prefix="", act=torch.relu, pre=None):
    """mixture_of_experts.py:101-162 written out: (B, N, E) -> (B, G, K); parameters by state_dict key under ``prefix``"""
    x2 = x.reshape(x.shape[0], -1)
    outs, i = [], 0
    while f"{prefix}experts.Expert_{i}.model.LinearOutput.weight" in P:
        outs.append(mlp(x2, P, f"{prefix}experts.Expert_{i}", act, pre))
        i += 1
    Ws, bs, g = [], [], 0
    while f"{prefix}gates.Gate_{g}.Linear.weight" in P:
        Ws.append(P[f"{prefix}gates.Gate_{g}.Linear.weight"])
        bs.append(P[f"{prefix}gates.Gate_{g}.Linear.bias"])
        g += 1
    return moe_gate(x2, torch.cat(Ws), torch.cat(bs), torch.cat(outs, dim=1))


def mmoe(x, P, pre=None):
    """multigate_moe.py:79-116: (B, N, E) -> (B, 1), the towers' outputs summed"""
    gated = moe_layer(x, P, "moe_layer.", pre=pre)
    out, t = 0, 0
    while f"towers.Tower_{t}.model.LinearOutput.weight" in P:
        out = out + mlp(gated[:, t], P, f"towers.Tower_{t}", pre=pre)
        t += 1
    return out


def deep_moe(x, P, pre=None):
    """deep_moe.py:68-92: stacked MoE layers, each output read as (B, 1, K), then the sum over K -> (B, 1)"""
    i = 0
    while f"module.{i}.gates.Gate_0.Linear.weight" in P:
        x = moe_layer(x, P, f"module.{i}.", pre=pre)
        i += 1
    return x.sum(dim=2)


def kink_margin(pre):
    """smallest |pre-activation| over the collected list"""
    return min(float(t.detach().abs().min()) for t in pre)
