"""The weight and input recipe of the ResNet golden (tools/gen_golden_resnet.py writes it from the reference's class, tests/test_resnet_host.py
and tests/test_gpu_resnet.py fill this package's class with the same values): helpers.seeded_fill on the floating-point entries with
seed 5, every `running_var` set to 0.5 + 5 |v| (seeded_fill's values would be negative half of the time, and with small variances the
network overflows by the second stage), `num_batches_tracked` 0; inputs are randn from ONE generator with seed 3."""
import torch

import helpers

WSEED, ISEED = 5, 3
SHAPE = (1, 3, 40, 72)          # stages 10x18, 5x9, 3x5, 2x3: an odd size at every level


def fill(state_dict):
    """{key: tensor} for every key of `state_dict` (a module's own: shapes and dtypes are read from it)"""
    sd = helpers.seeded_fill({k: tuple(v.shape) for k, v in state_dict.items() if v.is_floating_point()}, WSEED)
    for k, v in state_dict.items():
        if k.endswith("running_var"):
            sd[k] = 0.5 + 5.0 * sd[k].abs()
        elif not v.is_floating_point():
            sd[k] = torch.zeros_like(v)
    return sd


def inputs(n=1, shape=SHAPE):
    """the first n inputs of the generator: inputs(1)[0] is the golden's input, inputs(2)[1] the second one the tool compares with"""
    g = torch.Generator().manual_seed(ISEED)
    return [torch.randn(shape, generator=g) for _ in range(n)]
