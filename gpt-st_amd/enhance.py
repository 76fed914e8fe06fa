"""Downstream consumer of the pretrained encoder: the reference's ``Enhance_model.forward_pretrain`` +
``Fusion`` (model/Model.py:5-18, 20-46, 91-107) without the predictor zoo.  The frozen GPT-ST encoder (``mode='eval'``:
``dim_in_flow`` + one STHCN, no masking) runs on the HIP kernels; ``lin_test`` and the ``Fusion`` gate keep the reference's parameters
(state_dict keys) and run as one fused HIP launch (round 4, fusion.py) with a torch fallback, so any predictor (an ``nn.Module`` taking the (B,T,N,C)
embedding) can be trained on top with ordinary autograd."""
import torch
import torch.nn as nn

from .fusion import fusion_gate
from .model import GPTST_Model, _on_encoder_path


class Fusion(nn.Module):                                                   # model/Model.py:5-18
    def __init__(self, dim):
        super().__init__()
        self.HS_fc = nn.Linear(dim, dim, bias=True)
        self.HT_fc = nn.Linear(dim, dim, bias=True)
        self.output_fc = nn.Linear(dim, dim, bias=True)

    def forward(self, flow_eb, time_eb):
        z = torch.sigmoid(self.HS_fc(flow_eb) + self.HT_fc(time_eb))
        return self.output_fc(z * flow_eb + (1 - z) * time_eb)


def xavier_downstream_(model):
    """The reference Run.py:79-85 in eval mode: ``xavier_uniform_`` for dim > 1, else ``uniform_``, in ``named_parameters`` order, over what is
    trained on top of the pretrained encoder — the fusion gate, ``lin_test`` and the predictor.  Never the encoder: in the reference it is frozen
    when the pass runs; under ``finetune_encoder`` its parameters do require gradients here, and re-drawing them would throw the pretraining away."""
    for k, p in model.named_parameters():
        if p.requires_grad and not k.startswith("pretrain_model."):
            nn.init.xavier_uniform_(p) if p.dim() > 1 else nn.init.uniform_(p)
    return model


class EnhanceFrontEnd(nn.Module):
    """``Enhance_model`` in ``mode='eval'`` (model/Model.py:40-46,91-107): frozen pretrained encoder -> fusion with a linear lift
    of the raw flow -> predictor.  ``predictor=None`` returns the fused embedding.  ``finetune_encoder=True`` unfreezes the encoder path
    (``encoder.dim_in_flow`` and ``encoder.STHCN_encode``; the guide network and the decoder stay frozen): gradients reach it through the gate
    (fusion.py) and the encoder's own HIP backward (model._EncoderFn)."""

    def __init__(self, args, predictor=None, finetune_encoder=False):
        super().__init__()
        assert args.mode == "eval", "the enhanced front end wraps the encoder in eval mode (reference Run.py -mode eval)"
        self.input_base_dim = args.input_base_dim
        self.finetune_encoder = bool(finetune_encoder)
        self.pretrain_model = GPTST_Model(args)
        self.pretrain_model.finetune = self.finetune_encoder
        for k, p in self.pretrain_model.named_parameters():                # :93-94; fine-tuning: what the embedding depends on is trained too
            p.requires_grad = self.finetune_encoder and _on_encoder_path(k)
        self.fusion = Fusion(args.hidden_dim)
        self.lin_test = nn.Linear(args.input_base_dim, args.hidden_dim)
        self.predictor = predictor

    def load_pretrained_model(self, path_or_state):                        # :91-92
        sd = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, str) else path_or_state
        self.pretrain_model.load_state_dict(sd)

    def forward(self, source, label=None, batch_seen=None):                # :96-107
        x_pretrain_flow = self.pretrain_model(source, label)[0]
        # :105-107 lin_test + Fusion: one HIP launch forward (csrc/fusion.hip) where the shape allows, the torch modules otherwise
        if not self.finetune_encoder:
            x_pretrain_flow = x_pretrain_flow.detach()
        eb = fusion_gate(x_pretrain_flow, source, self.fusion, self.lin_test, self.input_base_dim)
        if self.predictor is None:
            return eb
        if getattr(self.predictor, "takes_targets", False):                # :110-114 (CCRNN): the labels feed the decoder's teacher forcing
            x = self.predictor(eb, None if label is None else label[..., :self.input_base_dim], None)
        else:
            x = self.predictor(eb)
        return x, x, x, x, x
