"""Downstream predictors trained on the enhanced embedding.  Not part of the pretraining hot path: they are
ordinary ``torch.nn`` modules on the GPU (rocBLAS / MIOpen through PyTorch-ROCm) behind the frozen HIP encoder of ``enhance.py``; each can
run the same parameters on the project's own kernels instead (``backend="hip"``: stgcn_hip.py, tgcn_hip.py, mtgnn_hip.py, astgcn_hip.py, stsgcn_hip.py, stfgnn_hip.py, stgode_hip.py, msdr_hip.py, stwa_hip.py, stmgcn_hip.py, ccrnn_hip.py, dmvstnet_hip.py)."""
from .stgcn import STGCN   # noqa: F401
from .tgcn import TGCN     # noqa: F401
from .mtgnn import MTGNN   # noqa: F401
from .astgcn import ASTGCN   # noqa: F401
from .stsgcn import STSGCN   # noqa: F401
from .stfgnn import STFGNN   # noqa: F401
from .stgode import STGODE   # noqa: F401
from .msdr import MSDR   # noqa: F401
from .stwa import STWA   # noqa: F401
from .stmgcn import STMGCN   # noqa: F401
from .ccrnn import CCRNN   # noqa: F401
from .dmvstnet import DMVSTNET   # noqa: F401
