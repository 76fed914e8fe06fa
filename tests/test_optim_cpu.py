"""CPU: the 13 host scalars of one fused clip + Adam step (ops.adam_scalars), as the fused stepper and ClipAdam hand them to gptst_clip_adam."""
import math

import numpy as np
import pytest

from gptst_amd import ops

B1, B2, EPS, LR, CLIP = 0.9, 0.999, 1e-8, 0.003, 5.0          # Run.py:134 (torch.optim.Adam defaults), PEMS08.conf: lr_init, max_grad_norm


def _words(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("tA,tB", [(1, 0), (1, 1), (7, 3), (1000, 400)])
def test_adam_scalars_are_the_words_the_stepper_and_clipadam_wrote(tA, tB):
    """bit for bit the float32 words of the two hand-written tuples this function replaced (kept here as literal expressions): the bias
    corrections in double precision, 1 - beta as the HOST rounds it (1.f - 0.999f on the device is 1.3e-5 low), KL path off before its first step"""
    b1, b2 = B1, B2
    kl = tB > 0
    # PretrainStep._fill: hyper[:11], then hyper[11:13]; the backward carries the gradient of the SUM loss (hyper[9] = 1)
    stepper = (LR / (1 - b1 ** tA), math.sqrt(1 - b2 ** tA),
               LR / (1 - b1 ** tB) if tB else 0.0, math.sqrt(1 - b2 ** tB) if tB else 1.0,
               b1, b2, 1e-8, CLIP, 1.0 if kl else 0.0,
               1.0,
               1.0) + (1 - b1, 1 - b2)
    assert _words(ops.adam_scalars(LR, tA, tB, B1, B2, EPS, CLIP, kl=kl, sum_loss=True)) == _words(stepper)
    # ClipAdam.step: autograd's gradient is that of the MEAN loss (hyper[9] = 0)
    clipadam = (LR / (1 - b1 ** tA), math.sqrt(1 - b2 ** tA), LR / (1 - b1 ** tB) if tB else 0.0, math.sqrt(1 - b2 ** tB) if tB else 1.0,
                b1, b2, EPS, CLIP, 1.0 if kl else 0.0, 0.0, 1.0, 1 - b1, 1 - b2)
    assert _words(ops.adam_scalars(LR, tA, tB, B1, B2, EPS, CLIP, kl=kl, sum_loss=False)) == _words(clipadam)
    assert len(stepper) == len(clipadam) == 13
    assert _words([1 - b2])[0] != _words([np.float32(1) - np.float32(b2)])[0]          # the subtlety is real: the two roundings differ
