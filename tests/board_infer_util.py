"""Nets, inputs and references shared by the one-launch TicTacToe inference tests (test_board_infer_*.py)."""

import copy

import torch

from handyrl_amd.envs.tictactoe import SimpleConv2dModel


EXACT_EPS = 2.0 ** -10


def seeded_net(layers=3, seed=0):
    """A SimpleConv2dModel(32, layers) in eval mode whose BatchNorm running statistics and affine parameters are
    off their initial values."""
    g = torch.Generator().manual_seed(1000 + seed)
    torch.manual_seed(seed)
    net = SimpleConv2dModel(32, layers)
    with torch.no_grad():
        for blk in net.blocks:
            blk.bn.running_mean.copy_(0.1 * torch.randn(32, generator=g))
            blk.bn.running_var.copy_(0.5 + torch.rand(32, generator=g))
            blk.bn.weight.copy_(0.75 + 0.5 * torch.rand(32, generator=g))
            blk.bn.bias.copy_(0.1 * torch.randn(32, generator=g))
    return net.eval()


def _sparse_int(shape, density, g):
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).float()


def integer_net(layers=3, seed=0):
    """A net on which every intermediate of the eval forward is exact in fp32 (and so equal in fp32 and fp64):
    conv weights in {-1, 0, 1}, most of them zero; BatchNorm weight a power of two <= 1, bias a small integer,
    running_mean an integer, running_var + eps exactly 1 (invstd exactly 1; torch refuses eps = 0, so running_var is
    1 - 2^-10 and eps 2^-10, whose sum is 1 in fp32 and in fp64); head conv biases large enough that every
    pre-activation is >= 0 (LeakyReLU the identity); integer fc weights, the value's summing to zero so that the
    value pre-activation stays where tanh is not saturated."""
    g = torch.Generator().manual_seed(2000 + seed)
    net = SimpleConv2dModel(32, layers)
    with torch.no_grad():
        net.conv.weight.copy_(_sparse_int(net.conv.weight.shape, 0.3, g))
        net.conv.bias.copy_(torch.randint(-1, 2, (32,), generator=g).float())
        for i, blk in enumerate(net.blocks):
            blk.conv.weight.copy_(_sparse_int(blk.conv.weight.shape, 0.04, g))
            last = i == layers - 1
            blk.bn.weight.copy_(torch.full((32,), 0.125) if last else
                                0.5 ** torch.randint(0, 2, (32,), generator=g).float())
            blk.bn.bias.copy_(torch.randint(-1, 3, (32,), generator=g).float())
            blk.bn.running_mean.copy_(torch.randint(-2, 3, (32,), generator=g).float())
            blk.bn.running_var.fill_(1.0 - EXACT_EPS)
            blk.bn.eps = EXACT_EPS
        for head in (net.head_p, net.head_v):
            head.conv.conv.weight.copy_(_sparse_int(head.conv.conv.weight.shape, 0.2, g))
            head.conv.conv.bias.fill_(64.0)
        net.head_p.fc.weight.copy_(torch.randint(-2, 3, net.head_p.fc.weight.shape, generator=g).float())
        net.head_v.fc.weight.copy_(torch.tensor([[1., -1., 0., 1., -1., 0., 1., -1., 0.]]))
    return net.eval()


def planes(n, seed=0):
    """0/1 observation planes (n, 3, 3, 3)."""
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randint(0, 2, (n, 3, 3, 3), generator=g).float()


def floats(n, seed=0):
    """General floats in [-2, 2]."""
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.rand(n, 3, 3, 3, generator=g) * 4 - 2


def quarters(n, seed=0):
    """Multiples of 1/4 in [-2, 2] (exact inputs that are not 0/1)."""
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randint(-8, 9, (n, 3, 3, 3), generator=g).float() / 4


@torch.no_grad()
def forward64(net, obs):
    """The fp64 torch-CPU forward of a deep copy of ``net`` in eval mode: (policy, value) as fp64."""
    ref = copy.deepcopy(net).cpu().double().eval()
    out = ref(obs.detach().cpu().double(), None)
    return out['policy'], out['value']


@torch.no_grad()
def value_preact64(net, obs):
    """The value head's pre-tanh output in fp64."""
    ref = copy.deepcopy(net).cpu().double().eval()
    h = torch.relu(ref.conv(obs.detach().cpu().double()))
    for blk in ref.blocks:
        h = torch.relu(blk(h))
    return ref.head_v(h)


@torch.no_grad()
def head_preacts64(net, obs):
    """Both heads' 1x1 conv outputs (before LeakyReLU) in fp64."""
    ref = copy.deepcopy(net).cpu().double().eval()
    h = torch.relu(ref.conv(obs.detach().cpu().double()))
    for blk in ref.blocks:
        h = torch.relu(blk(h))
    return ref.head_p.conv(h), ref.head_v.conv(h)
