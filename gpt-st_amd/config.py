"""Flag/config system for ``-mode pretrain`` (mirrors reference lib/Params_pretrain.py:6-77).

Two-stage parse like the reference: stage 1 reads ``-dataset/-mode/-device/-model``,
stage 2 loads ``conf/GPTST_pretrain/<dataset>.conf`` and registers every key as a
single-dash flag whose default is the INI value.  Unlike the reference the conf path is
resolved relative to this package (not the CWD) and no predictor conf is read
(reference Run.py:36 reads one and never uses it in pretrain mode).
"""
import argparse
import configparser
import os
from types import SimpleNamespace

CONF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conf", "GPTST_pretrain")

# dataset -> (interval minutes, week_day) as set by reference lib/load_dataset.py:50-53,61-64,73-77,85-89
DATASET_TIME = {"PEMS08": (5, 7), "METR_LA": (5, 7), "NYC_BIKE": (30, 7), "NYC_TAXI": (30, 7)}

_EVAL = lambda s: eval(s) if isinstance(s, str) else s  # noqa: E731  (reference uses type=eval for bools/None)

# (section, key, type) in the reference's registration order (Params_pretrain.py:26-74)
_KEYS = [
    ("data", "val_ratio", float), ("data", "test_ratio", float), ("data", "lag", int), ("data", "horizon", int),
    ("data", "num_nodes", int), ("data", "tod", _EVAL), ("data", "normalizer", str), ("data", "column_wise", _EVAL),
    ("data", "default_graph", _EVAL),
    ("model", "input_base_dim", int), ("model", "input_extra_dim", int), ("model", "output_dim", int),
    ("model", "embed_dim", int), ("model", "embed_dim_spa", int), ("model", "hidden_dim", int), ("model", "HS", int),
    ("model", "HT", int), ("model", "HT_Tem", int), ("model", "num_route", int), ("model", "mask_ratio", float),
    ("model", "ada_mask_ratio", float), ("model", "ada_type", str),
    ("train", "loss_func", str), ("train", "seed", int), ("train", "batch_size", int), ("train", "epochs", int),
    ("train", "lr_init", float), ("train", "lr_decay", _EVAL), ("train", "lr_decay_rate", float),
    ("train", "lr_decay_step", str), ("train", "early_stop", _EVAL), ("train", "early_stop_patience", int),
    ("train", "change_epoch", int), ("train", "up_epoch", str), ("train", "grad_norm", _EVAL),
    ("train", "max_grad_norm", int), ("train", "debug", _EVAL), ("train", "real_value", _EVAL),
    ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "load_pretrain_path", str),
    ("train", "save_pretrain_path", str),
    ("test", "mae_thresh", _EVAL), ("test", "mape_thresh", float),
    ("log", "log_step", int), ("log", "plot", _EVAL),
]


def _read_conf(dataset):
    path = os.path.join(CONF_DIR, "%s.conf" % dataset)
    if not os.path.isfile(path):
        raise FileNotFoundError("no pretrain conf for dataset %r (looked in %s)" % (dataset, CONF_DIR))
    cp = configparser.ConfigParser()
    cp.optionxform = str  # keep HS/HT/HT_Tem case
    cp.read(path)
    return cp


def parse_args(device, argv=None):
    """Same flag surface as reference ``parse_args(device)`` for the pretrain set."""
    ap = argparse.ArgumentParser(prefix_chars="-", description="pretrain_arguments")
    ap.add_argument("-dataset", default="METR_LA", type=str, required=True)
    ap.add_argument("-mode", default="ori", type=str, required=True)
    ap.add_argument("-device", default=device, type=str)
    ap.add_argument("-model", default="TGCN", type=str)
    ap.add_argument("-cuda", default=True, type=bool)
    first, _ = ap.parse_known_args(argv)
    cp = _read_conf(first.dataset)
    for sec, key, typ in _KEYS:
        ap.add_argument("-" + key, default=typ(cp[sec][key]), type=typ)
    ap.add_argument("-log_dir", default="./", type=str)
    ap.add_argument("-steps_per_replay", default=STEPS_PER_REPLAY, type=int)      # not a reference option: see STEPS_PER_REPLAY
    # not a reference option: what the ranks of a torch.distributed.run job split — the batch (data parallel) or the nodes (shard.py)
    ap.add_argument("-shard", default="batch", choices=["batch", "nodes"], type=str)
    # not reference options: the run's state in one portable file (checkpoint.py), written every N epochs and read back by -resume
    ap.add_argument("-ckpt_every", default=CKPT_DEFAULTS["ckpt_every"], type=int)      # epochs between checkpoints; 0 writes none
    ap.add_argument("-ckpt_path", default=CKPT_DEFAULTS["ckpt_path"], type=str)        # '' = <log_dir>/pretrain_state.pth; may contain {epoch}
    ap.add_argument("-resume", default=CKPT_DEFAULTS["resume"], type=str)              # '' = start fresh, 'auto' = ckpt_path if that file exists
    # not reference options: -mode eval trains the pretrained encoder too (enhance.EnhanceFrontEnd), at lr_init * encoder_lr_scale
    ap.add_argument("-finetune_encoder", default=FINETUNE_DEFAULTS["finetune_encoder"], type=_EVAL)
    ap.add_argument("-encoder_lr_scale", default=FINETUNE_DEFAULTS["encoder_lr_scale"], type=float)
    # not a reference option: what runs the STGCN predictor of -mode eval: the torch modules or the HIP kernels (predictors/stgcn_hip.py)
    ap.add_argument("-stgcn_backend", default=FINETUNE_DEFAULTS["stgcn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the TGCN predictor (predictors/tgcn_hip.py)
    ap.add_argument("-tgcn_backend", default=FINETUNE_DEFAULTS["tgcn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the MTGNN predictor (predictors/mtgnn_hip.py)
    ap.add_argument("-mtgnn_backend", default=FINETUNE_DEFAULTS["mtgnn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the ASTGCN predictor (predictors/astgcn_hip.py)
    ap.add_argument("-astgcn_backend", default=FINETUNE_DEFAULTS["astgcn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the STSGCN predictor (predictors/stsgcn_hip.py)
    ap.add_argument("-stsgcn_backend", default=FINETUNE_DEFAULTS["stsgcn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the STFGNN predictor (predictors/stfgnn_hip.py)
    ap.add_argument("-stfgnn_backend", default=FINETUNE_DEFAULTS["stfgnn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the STGODE predictor (predictors/stgode_hip.py)
    ap.add_argument("-stgode_backend", default=FINETUNE_DEFAULTS["stgode_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the MSDR predictor (predictors/msdr_hip.py)
    ap.add_argument("-msdr_backend", default=FINETUNE_DEFAULTS["msdr_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the ST-WA predictor (predictors/stwa_hip.py)
    ap.add_argument("-stwa_backend", default=FINETUNE_DEFAULTS["stwa_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the ST-MGCN predictor (predictors/stmgcn_hip.py)
    ap.add_argument("-stmgcn_backend", default=FINETUNE_DEFAULTS["stmgcn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the CCRNN predictor (predictors/ccrnn_hip.py)
    ap.add_argument("-ccrnn_backend", default=FINETUNE_DEFAULTS["ccrnn_backend"], choices=["torch", "hip"], type=str)
    # not a reference option: the same choice for the DMVSTNET predictor (predictors/dmvstnet_hip.py)
    ap.add_argument("-dmvstnet_backend", default=FINETUNE_DEFAULTS["dmvstnet_backend"], choices=["torch", "hip"], type=str)
    args, _ = ap.parse_known_args(argv)
    args.interval, args.week_day = DATASET_TIME.get(args.dataset, (5, 7))
    return args


# Optimisation steps enqueued per hipGraph replay by the trainer and bench.py (PretrainStep.step_group): the device idles ~19 us between
# two graph replays, one replay per 4 steps removes three quarters of that.  1 = one replay per step.  Results do not depend on it.
STEPS_PER_REPLAY = int(os.environ.get("GPTST_STEPS_PER_REPLAY", "4"))


CKPT_DEFAULTS = dict(ckpt_every=0, ckpt_path="", resume="")
FINETUNE_DEFAULTS = dict(finetune_encoder=False, encoder_lr_scale=1.0, stgcn_backend="torch", tgcn_backend="torch", mtgnn_backend="torch",
                         astgcn_backend="torch", stsgcn_backend="torch", stfgnn_backend="torch", stgode_backend="torch",
                         msdr_backend="torch", stwa_backend="torch", stmgcn_backend="torch", ccrnn_backend="torch",
                         dmvstnet_backend="torch")


def make_args(dataset="PEMS08", mode="pretrain", device="cpu", **overrides):
    """Programmatic equivalent of ``parse_args`` (used by tests, bench and golden scripts)."""
    cp = _read_conf(dataset)
    ns = SimpleNamespace(dataset=dataset, mode=mode, device=device, model="TGCN", cuda=True, log_dir="./")
    for sec, key, typ in _KEYS:
        setattr(ns, key, typ(cp[sec][key]))
    ns.interval, ns.week_day = DATASET_TIME.get(dataset, (5, 7))
    ns.scaler_zeros = 0.0
    ns.steps_per_replay = STEPS_PER_REPLAY
    for k, v in list(CKPT_DEFAULTS.items()) + list(FINETUNE_DEFAULTS.items()):
        setattr(ns, k, v)
    for k, v in overrides.items():
        setattr(ns, k, v)
    return ns


# ---- downstream predictors (-mode eval): reference lib/Params_predictor.py:4-25 + model/STGCN/args.py:52-76 -------------------------
PRED_CONF = os.path.join(os.path.dirname(CONF_DIR), "GPTST_pretrain", "params_predictors.conf")
_PRED_TRAIN = [("batch_size", int), ("epochs", int), ("lr_init", float), ("lr_decay", _EVAL), ("lr_decay_rate", float), ("lr_decay_step", str),
               ("early_stop", _EVAL), ("early_stop_patience", int), ("grad_norm", _EVAL), ("max_grad_norm", int), ("debug", _EVAL),
               ("real_value", _EVAL)]
_STGCN_KEYS = [("data", "num_nodes", int), ("data", "input_window", int), ("data", "output_window", int), ("model", "Ks", int),
               ("model", "Kt", int), ("model", "blocks1", _EVAL), ("model", "drop_prob", int), ("model", "outputl_ks", int),
               ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/TGCN/args.py:14-25.  `lam` is parsed and, as in the reference (TGCN.py:140 stores it, nothing reads it), used nowhere.
_TGCN_KEYS = [("data", "num_nodes", int), ("data", "input_window", int), ("data", "output_window", int), ("model", "rnn_units", int),
              ("model", "lam", float), ("model", "output_dim", int),
              ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/MTGNN/args.py:13-39.  `use_curriculum_learning` and `task_level` are parsed and, as in the reference, read by nothing.
_MTGNN_KEYS = [("data", "num_nodes", int), ("data", "input_window", int), ("data", "output_window", int), ("data", "output_dim", int),
               ("model", "gcn_true", _EVAL), ("model", "buildA_true", _EVAL), ("model", "gcn_depth", int), ("model", "dropout", float),
               ("model", "subgraph_size", int), ("model", "node_dim", int), ("model", "dilation_exponential", int),
               ("model", "conv_channels", int), ("model", "residual_channels", int), ("model", "skip_channels", int),
               ("model", "end_channels", int), ("model", "layers", int), ("model", "propalpha", float), ("model", "tanhalpha", int),
               ("model", "layer_norm_affline", _EVAL), ("model", "use_curriculum_learning", _EVAL), ("model", "task_level", int),
               ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/ASTGCN/args.py.  `xavier` is True in all four confs: the attention and Theta parameters have no other initialisation.
_ASTGCN_KEYS = [("data", "num_nodes", int), ("data", "len_input", int), ("data", "num_for_predict", int), ("model", "nb_block", int),
                ("model", "K", int), ("model", "nb_chev_filter", int), ("model", "nb_time_filter", int), ("model", "time_strides", int),
                ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/STSGCN/args.py:12-35.  `filter_list` is a literal (a list of lists of widths); `rho` is parsed and, as in the reference, read by nothing.
_STSGCN_KEYS = [("data", "num_nodes", int), ("data", "input_window", int), ("data", "output_window", int), ("model", "filter_list", _EVAL),
                ("model", "rho", int), ("model", "feature_dim", int), ("model", "module_type", str), ("model", "activation", str),
                ("model", "temporal_emb", _EVAL), ("model", "spatial_emb", _EVAL), ("model", "use_mask", _EVAL), ("model", "steps", int),
                ("model", "first_layer_embedding_size", int),
                ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/STFGNN/args.py:165-187.  `hidden_dims` is a literal (a list of lists of widths); `order`, `lag`, `period`, `sparsity` and
# `module_type` are parsed and, as in the reference, read by nothing in the model.
_STFGNN_KEYS = [("data", "num_nodes", int), ("data", "window", int), ("data", "horizon", int), ("data", "order", int), ("data", "lag", int),
                ("data", "period", int), ("data", "sparsity", float), ("model", "hidden_dims", _EVAL),
                ("model", "first_layer_embedding_size", int), ("model", "out_layer_dim", int), ("model", "output_dim", int),
                ("model", "strides", int), ("model", "temporal_emb", _EVAL), ("model", "spatial_emb", _EVAL), ("model", "use_mask", _EVAL),
                ("model", "activation", str), ("model", "module_type", str),
                ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/STGODE/args.py:156-171.  `out_channels` is a literal (the widths of a temporal block; the last is a block's output width).
_STGODE_KEYS = [("data", "num_nodes", int), ("data", "num_timesteps_input", int), ("data", "num_timesteps_output", int),
                ("model", "sigma1", float), ("model", "sigma2", float), ("model", "thres1", float), ("model", "thres2", float),
                ("model", "in_channels", int), ("model", "out_channels", _EVAL), ("model", "n_layers", int),
                ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/MSDR/args.py:90-109.  ``filter_type`` takes its default from the conf's ``cl_decay_steps`` as the reference does (args.py:90): the
# string "2000", which no branch of the cell names, so the confs' own ``dual_random_walk`` is never read and the cell runs on one scaled Laplacian
# (graph.msdr_supports); ``--filter_type dual_random_walk`` on the command line selects the others.  `cl_decay_steps`, `use_curriculum_learning`,
# `construct_type` and `l2lambda` are parsed and, as in the reference, read by nothing; `input_dim` is not read at all (Model.py:81 sets dim_in).
_MSDR_KEYS = [("model", "cl_decay_steps", str, "filter_type"), ("model", "cl_decay_steps", int), ("model", "num_nodes", int),
              ("model", "horizon", int), ("model", "seq_len", int), ("model", "max_diffusion_step", int), ("model", "num_rnn_layers", int),
              ("model", "output_dim", int), ("model", "rnn_units", int), ("model", "pre_k", int), ("model", "pre_v", int),
              ("model", "use_curriculum_learning", _EVAL), ("model", "construct_type", str), ("model", "l2lambda", int),
              ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/ST_WA/args.py:41-55.  ``dynamic`` is a string there (``type=str``): every conf value, "False" included, is truthy, so the
# static branch of the model is dead; it is parsed the same way and predictors.STWA refuses the one falsy value, the empty string.  `in_dim`
# is parsed and, as in the reference (Model.py:78 sets dim_in), read by nothing.  The adjacency of args.py:60-71 is read by nothing either.
_STWA_KEYS = [("data", "num_nodes", int), ("data", "lag", int), ("data", "horizon", int), ("model", "in_dim", int), ("model", "out_dim", int),
              ("model", "channels", int), ("model", "dynamic", str), ("model", "memory_size", int),
              ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
# reference model/STMGCN_demand/args.py:16-29.  `gconv_activation` is parsed and, as in the reference (STMGCN.py:71 leaves it commented out),
# read by nothing: the graph convolutions apply ReLU always.  The reference serves the two demand datasets only (STMGCN_DATASETS).
_STMGCN_KEYS = [("data", "seq_len", int), ("data", "M", int), ("data", "n_nodes", int), ("model", "lstm_hidden_dim", int),
                ("model", "lstm_num_layers", int), ("model", "gcn_hidden_dim", int), ("model", "gconv_use_bias", _EVAL),
                ("model", "gconv_activation", str),
                ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
STMGCN_DATASETS = ("NYC_TAXI", "NYC_BIKE")
# reference model/CCRNN_demand/args.py:89-109.  `num_input` and `Normal_Method` are parsed and read by the support's construction alone
# (Run.py ccrnn_support); `input_dim` and `output_dim` are parsed and, as in the reference (Model.py:88 sets dim_in and dim_out), read by nothing.
_CCRNN_KEYS = [("data", "Normal_Method", str), ("data", "normalized_category", str), ("data", "hidden_size_data", int), ("data", "num_input", int),
               ("data", "num_predict", int), ("data", "num_nodes", int), ("model", "hidden_size", int), ("model", "n_dim", int),
               ("model", "n_supports", int), ("model", "k_hop", int), ("model", "n_rnn_layers", int), ("model", "n_gconv_layers", int),
               ("model", "input_dim", int), ("model", "output_dim", int), ("model", "cl_decay_steps", int),
               ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
CCRNN_DATASETS = ("NYC_TAXI", "NYC_BIKE")
# reference model/DMVSTNET_demand/args.py:16-26.  `output_window` is parsed and, as in the reference, read by nothing in the model: the output has
# input_window steps.  The reference's confs carry nine more [model] keys (cnn_hidden_dim_first, local_image_size, ...) that its args.py never parses.
_DMVSTNET_KEYS = [("data", "input_window", int), ("data", "output_window", int), ("data", "num_nodes", int), ("model", "hidden_dim", int),
                  ("model", "topo_embedded_dim", int),
                  ("train", "seed", int), ("train", "seed_mode", _EVAL), ("train", "xavier", _EVAL), ("train", "loss_func", str)]
DMVSTNET_DATASETS = ("NYC_TAXI", "NYC_BIKE")
_PRED_KEYS = {"STGCN": _STGCN_KEYS, "TGCN": _TGCN_KEYS, "MTGNN": _MTGNN_KEYS, "ASTGCN": _ASTGCN_KEYS, "STSGCN": _STSGCN_KEYS,
              "STFGNN": _STFGNN_KEYS, "STGODE": _STGODE_KEYS, "MSDR": _MSDR_KEYS, "STWA": _STWA_KEYS, "STMGCN": _STMGCN_KEYS, "CCRNN": _CCRNN_KEYS,
              "DMVSTNET": _DMVSTNET_KEYS}
_PRED_DIRS = {"STWA": "ST-WA", "STMGCN": "STMGCN_demand", "CCRNN": "CCRNN_demand", "DMVSTNET": "DMVSTNET_demand"}               # the conf directory where it is not the model's name (the reference's own spelling)


def predictor_args(dataset, model="STGCN", argv=None):
    """The predictor's own argument set (double-dash flags as in the reference): the shared training schedule of
    params_predictors.conf, then conf/<model>/<dataset>.conf.  STGCN, TGCN, MTGNN, ASTGCN, STSGCN, STFGNN, STGODE, MSDR, STWA, STMGCN, CCRNN and DMVSTNET are built."""
    if model not in _PRED_KEYS:
        raise ValueError("gpt-st_amd builds the STGCN, TGCN, MTGNN, ASTGCN, STSGCN, STFGNN, STGODE, MSDR, STWA, STMGCN, CCRNN and DMVSTNET predictors only, got %r" % (model,))
    if model == "STMGCN" and dataset not in STMGCN_DATASETS:                      # reference model/STMGCN_demand/args.py:8-9, before any conf is read
        raise ValueError("Demand prediction baseline. Please select NYC_TAXI or NYC_BIKE dataset!")
    if model == "CCRNN" and dataset not in CCRNN_DATASETS:                        # reference model/CCRNN_demand/args.py:80-81, likewise
        raise ValueError("Demand prediction baseline. Please select NYC_TAXI or NYC_BIKE dataset!")
    if model == "DMVSTNET" and dataset not in DMVSTNET_DATASETS:                  # reference model/DMVSTNET_demand/args.py:7-8, likewise
        raise ValueError("Demand prediction baseline. Please select NYC_TAXI or NYC_BIKE dataset!")
    cp = configparser.ConfigParser()
    cp.optionxform = str
    cp.read(PRED_CONF)
    ap = argparse.ArgumentParser(prefix_chars="--", description="predictor_based_arguments")
    for key, typ in _PRED_TRAIN:
        ap.add_argument("--" + key, default=typ(cp["train"][key]), type=typ)
    path = os.path.join(os.path.dirname(CONF_DIR), _PRED_DIRS.get(model, model), "%s.conf" % dataset)
    if not os.path.isfile(path):
        raise FileNotFoundError("no %s conf for dataset %r (%s)" % (model, dataset, path))
    cm = configparser.ConfigParser()
    cm.optionxform = str
    cm.read(path)
    for sec, key, typ, *flag in _PRED_KEYS[model]:                               # (a fourth entry: the flag that takes this conf key's value as its default)
        ap.add_argument("--" + (flag[0] if flag else key), default=typ(cm[sec][key]), type=typ)
    pargs, _ = ap.parse_known_args([] if argv is None else argv)
    return pargs


def apply_predictor_overrides(args, pargs):
    """reference Run.py:36-43: outside pretrain mode every attribute the predictor's argument set also has replaces the pretrain
    conf's value (batch_size 64, epochs 100, lr_decay_step 25,50,75, early_stop_patience 25, debug False, xavier False, seed, ...)."""
    for attr in list(vars(args)):
        if hasattr(pargs, attr):
            setattr(args, attr, getattr(pargs, attr))
    return args
