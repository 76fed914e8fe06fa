#!/usr/bin/env python
"""``python Run.py -dataset PEMS08 -mode pretrain [-key value ...]`` (and ``-mode eval -model STGCN | TGCN | MTGNN | ASTGCN | STSGCN | STFGNN | STGODE | MSDR | STWA | STMGCN | CCRNN | DMVSTNET``: a downstream predictor on the
enhanced embedding) — same flags as the reference model/Run.py for the
pretrain mode (reference Run.py:35,49,55-58,63-69,72-74,79-85,115-117,132-143,153-156).  Data: the reference's layout
``<root>/<DATASET>/<file>.npz`` with ``['data']`` of shape (L, N, F) under ``-data_root`` (default ../data, as in the reference),
loaded by gptst_amd.data (time indices, split, windows, z-score: parity-tested against the reference's loader functions);
when the file is absent a synthetic series of the dataset's shape is used (the data zips are not redistributable).
Multi-GPU: launch with torch.distributed.run (one process per GPU)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from gptst_amd import data as gdata, synth                   # noqa: E402
from gptst_amd.config import apply_predictor_overrides, parse_args, predictor_args   # noqa: E402
from gptst_amd.model import GPTST_Model, init_seed, xavier_init_   # noqa: E402
from gptst_amd.trainer import Trainer                        # noqa: E402


def load_series(args, dev):
    """-> (data_root, loaders + scalers of gdata.get_dataloader): the dataset under -data_root, or — when its file is absent — a synthetic
    series of the dataset's shape (METR_LA's file holds (L, N) without a channel axis, lib/load_dataset.py:57-60)."""
    extra = [a for a in sys.argv[1:]]
    data_root = extra[extra.index("-data_root") + 1] if "-data_root" in extra else "../data"
    fname = gdata.DATASETS[args.dataset][0]
    raw = None
    if not os.path.exists(os.path.join(data_root, fname)):                       # synthetic stand-in of the dataset's shape
        F = 3 if args.dataset == "PEMS08" else args.input_base_dim
        raw = synth.make_series(args.num_nodes, F, interval=gdata.DATASETS[args.dataset][2], seed=args.seed)
        if args.dataset == "METR_LA":
            raw = raw[..., 0]
        print("gpt-st_amd: %s not found -> synthetic %s-shaped series %s" % (os.path.join(data_root, fname), args.dataset, raw.shape))
    g = torch.Generator().manual_seed(args.seed)
    return data_root, gdata.get_dataloader(args, root=data_root, device=dev, raw=raw, generator=g)


EVAL_MODELS = ("STGCN", "TGCN", "MTGNN", "ASTGCN", "STSGCN", "STFGNN", "STGODE", "MSDR", "STWA", "STMGCN", "CCRNN", "DMVSTNET")      # what -mode eval builds


def main():
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    args = parse_args(str(dev))
    if args.mode == "eval" and args.shard == "nodes":
        raise SystemExit("-shard nodes applies to -mode pretrain only (-mode eval trains the predictor on one GPU)")
    if args.mode == "eval":
        return main_eval(args, dev)
    if args.mode != "pretrain":
        raise SystemExit("gpt-st_amd implements -mode pretrain and -mode eval -model STGCN | TGCN | MTGNN | ASTGCN | STSGCN | STFGNN | STGODE | MSDR | STWA | STMGCN | CCRNN | DMVSTNET")
    if args.shard == "nodes":
        return main_shard(args, dev)
    dp = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from gptst_amd.dist import DataParallel
        # per-step collectives on the C-ABI communicator (captured inside the step's hipGraph); GPTST_NATIVE_COMM=0: torch.distributed
        dp = DataParallel("nccl", native=os.environ.get("GPTST_NATIVE_COMM", "1") == "1" and os.environ.get("GPTST_DIST_BACKEND", "nccl") == "nccl")
    init_seed(args.seed)
    args.log_dir = os.path.join(os.path.dirname(os.path.realpath(__file__)), "SAVE", args.dataset)
    _, (train, val, test, scaler, _, _) = load_series(args, dev)
    mean, std = float(scaler.mean), float(scaler.std)
    args.scaler_zeros = float(scaler.transform(0))                               # Run.py:67
    model = GPTST_Model(args)
    if args.xavier:
        xavier_init_(model)
    model = model.to(dev)
    if dp is not None:
        dp.broadcast_(model.flat)

    batches, nb = gdata.epoch_batches(train, args.batch_size, dp)      # under data parallelism the epoch's tail is kept as padded rounds
    Trainer(model, args, batches, mean, std, args.batch_size, dp=dp, batches_per_epoch=nb, loader=train).train()      # (-resume: Trainer.train)
    if dp is not None:
        import torch.distributed as dist
        dp.barrier()
        dist.destroy_process_group()


def main_shard(args, dev):
    """``-mode pretrain -shard nodes``: every rank of the job owns a contiguous node range (shard.node_ranges) of every batch and of the
    node-indexed parameters; all ranks step on the same global batches.  The checkpoint is the global, reference-format state dict."""
    import copy
    from gptst_amd.shard import DistNodeGroup, NativeNodeGroup, node_ranges, shard_state_dict
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    ranges = node_ranges(args.num_nodes, world)          # (raises before any rendezvous when world > N)
    dp, group = None, DistNodeGroup(0, 1)
    if world > 1:
        from gptst_amd.dist import DataParallel
        # rendezvous as in the data-parallel branch; the collectives on the C-ABI communicator unless GPTST_NATIVE_COMM=0 / a gloo backend
        dp = DataParallel("nccl", native=os.environ.get("GPTST_NATIVE_COMM", "1") != "0" and os.environ.get("GPTST_DIST_BACKEND", "nccl") == "nccl")
        group = NativeNodeGroup(dp.native) if dp.native is not None else DistNodeGroup(rank, world)
    init_seed(args.seed)
    args.log_dir = os.path.join(os.path.dirname(os.path.realpath(__file__)), "SAVE", args.dataset)
    _, (train, val, test, scaler, _, _) = load_series(args, dev)       # GLOBAL N: the scaler is the global train split's
    mean, std = float(scaler.mean), float(scaler.std)
    args.scaler_zeros = float(scaler.transform(0))
    gmodel = GPTST_Model(args)                                          # the global initialisation, identical on every rank
    if args.xavier:
        xavier_init_(gmodel)
    n0, n1 = ranges[rank]
    largs = copy.copy(args)
    largs.num_nodes, largs.node_capacity = n1 - n0, max(b - a for a, b in ranges)
    model = GPTST_Model(largs)
    model.load_state_dict(shard_state_dict(gmodel.state_dict(), n0, n1))
    del gmodel
    model = model.to(dev)
    for ld in (train, val, test):                                       # the windows index time only: keep this rank's node columns
        if ld is not None:
            ld.series = ld.series[:, n0:n1].contiguous()
    batches, nb = gdata.epoch_batches(train, args.batch_size)          # same permutation on every rank: the same global batches
    Trainer(model, largs, batches, mean, std, args.batch_size, batches_per_epoch=nb, shard=(group, ranges), loader=train).train()
    if dp is not None:
        import torch.distributed as dist
        dp.barrier()
        dist.destroy_process_group()


def fusion_matrix(args, data_root, A, loaders, scaler):
    """STFGNN's (4N, 4N) spatial-temporal fusion graph (reference model/STFGNN/args.py:192-210): ``<data_root>/STFGNN/<ds>/<ds>_adj_mx.npy`` when
    that file exists; otherwise built from the adjacency and the DTW graph of the loaded series (graph.dtw_graph, on the series' device), and
    cached there as the reference does.  The series at hand is the training split, z-scored: the head of the data, longer than the 60 % of
    its days the DTW graph reads; it is put back to real values first, though the DTW normalises every day's row anyway."""
    from gptst_amd import graph
    path = os.path.join(data_root, "STFGNN", args.dataset, args.dataset + "_adj_mx.npy")
    if os.path.exists(path):
        return torch.tensor(np.load(path), dtype=torch.float32)
    series = loaders[0].series[:, :, 0] * float(scaler.std) + float(scaler.mean)
    whole = sum(ld.series.shape[0] for ld in loaders if ld is not None)
    print("gpt-st_amd: %s not found -> DTW graph of the %s training series %s" % (path, args.dataset, tuple(series.shape)), flush=True)
    dtw = graph.dtw_graph(series, args.dataset, total_steps=whole)
    adj = graph.stfgnn_fusion_graph(A, dtw)
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, adj.double().numpy())
    except OSError as e:
        print("gpt-st_amd: the fusion matrix is not cached (%s)" % e)
    return adj


def stgode_graphs(args, pargs, data_root, A, csv_path, train):
    """STGODE's spatial and semantic graphs (reference model/STGODE/args.py:44-131, 176-177) from ``<data_root>/STGODE/<ds>/<ds>_dtw_distance.npy``
    and ``_spatial_distance.npy`` when those files exist; otherwise the distances are built and cached there as the reference does: the
    spatial ones from the dataset's csv by the reference's per-dataset rules — where only an adjacency exists (the synthetic graph) by
    (1 - adj) 1000 — and the DTW ones between the day-mean profiles of the loaded, z-scored series with the project's exact recurrence (the
    reference approximates with fastdtw(radius=6)).  The series at hand is the training split where the reference averages the days of
    the whole series."""
    from gptst_amd import graph
    root = os.path.join(data_root, "STGODE", args.dataset)
    dist = {}
    for kind in ("dtw", "spatial"):
        path = os.path.join(root, "%s_%s_distance.npy" % (args.dataset, kind))
        if os.path.exists(path):
            dist[kind] = np.load(path)
            continue
        print("gpt-st_amd: %s not found -> built from the %s" % (path, "training series" if kind == "dtw" else "adjacency"), flush=True)
        if kind == "dtw":
            day = 288 if train.series.shape[0] >= 288 else int(train.series.shape[0])
            dist[kind] = graph.stgode_dtw_distances(train.series, day_slots=day)
        else:
            dist[kind] = (graph.stgode_spatial_distance_csv(csv_path, args.dataset, args.num_nodes) if os.path.exists(csv_path)
                          else graph.stgode_spatial_distance(A))
        try:
            os.makedirs(root, exist_ok=True)
            np.save(path, dist[kind])
        except OSError as e:
            print("gpt-st_amd: the %s distances are not cached (%s)" % (kind, e))
    return graph.stgode_graphs(dist["spatial"], dist["dtw"], pargs.sigma1, pargs.sigma2, pargs.thres1, pargs.thres2)


def stmgcn_graphs(args, data_root, A, train):
    """ST-MGCN's two Chebyshev support stacks (reference model/STMGCN_demand/args.py:35-53): the distance graph and the correlation graph of
    ``<data_root>/STMGCN_demand/{dis,pcc}_{tt|bb}.csv`` (comma-separated, no header) where those files exist.  Where one is absent — this
    fallback is the project's own, the reference has none — the distance graph is the adjacency at hand and the correlation graph the
    Pearson correlation between the nodes of the training series' first channel."""
    from gptst_amd import graph
    tag = {"NYC_TAXI": "tt", "NYC_BIKE": "bb"}[args.dataset]
    raw = {}
    for kind in ("dis", "pcc"):
        path = os.path.join(data_root, "STMGCN_demand", "%s_%s.csv" % (kind, tag))
        if os.path.exists(path):
            raw[kind] = np.loadtxt(path, delimiter=",", dtype=np.float32, ndmin=2)
            continue
        print("gpt-st_amd: %s not found -> built from the %s" % (path, "adjacency" if kind == "dis" else "training series"), flush=True)
        raw[kind] = (np.asarray(A, dtype=np.float32) if kind == "dis"
                     else graph.stmgcn_correlation(train.series[:, :, 0].detach().cpu().numpy()))
    return graph.stmgcn_supports(raw["dis"]), graph.stmgcn_supports(raw["pcc"])


CCRNN_HOLDOUT = 1700                 # reference CCRNN_demand/args.py:113,116: _len = [850, 850], the frames kept away from the support


def ccrnn_support(args, pargs, data_root, loaders, scaler, holdout=CCRNN_HOLDOUT):
    """CCRNN's (N, N) support (reference model/CCRNN_demand/args.py:40-76, 112-120) from the dataset's raw first two channels (pick-up and
    drop-off: the arrays the reference reads from its h5 files), all but the last ``holdout`` frames.  ``<data_root>/<ds>/<file>.npz`` where it
    exists; otherwise, or where the series is too short for that holdout — this fallback is the project's own, the reference has none — the
    training split of the loaded series put back to real values, whole."""
    from gptst_amd import graph
    path = os.path.join(data_root, gdata.DATASETS[args.dataset][0])
    series = None
    if os.path.exists(path):
        series = np.load(path)["data"][..., :2].astype(np.float64)
    if series is None or series.ndim != 3 or series.shape[-1] < 2 or series.shape[0] <= holdout:
        tr = loaders[0].series[:, :, :2].detach().cpu().double().numpy() * float(scaler.std) + float(scaler.mean)
        print("gpt-st_amd: CCRNN support from the %s training split %s alone (no raw series of more than %d frames at %s)"
              % (args.dataset, tuple(tr.shape), holdout, path), flush=True)
        return torch.tensor(graph.ccrnn_support(tr, pargs.hidden_size_data, pargs.normalized_category, 0), dtype=torch.float32)
    return torch.tensor(graph.ccrnn_support(series, pargs.hidden_size_data, pargs.normalized_category, holdout), dtype=torch.float32)


def dmvstnet_adjacency(args, csv_path, A):
    """DMVSTNET's graph (reference model/DMVSTNET_demand/args.py:32-33): the header-less N x N matrix of ``<data_root>/<DS>/<DS>.csv`` as it is,
    neither normalised nor thresholded.  Where the file is absent — this fallback is the project's own, the reference has none — the adjacency
    at hand."""
    from gptst_amd import graph
    if os.path.exists(csv_path):
        return torch.tensor(graph.dmvstnet_adjacency(csv_path, args.num_nodes))
    print("gpt-st_amd: %s not found -> DMVSTNET runs on the adjacency at hand" % csv_path, flush=True)
    return torch.tensor(np.asarray(A, dtype=np.float32))


def main_eval(args, dev):
    """``-mode eval -model STGCN | TGCN | MTGNN | ASTGCN | STSGCN | STFGNN | STGODE | MSDR | STWA | STMGCN | CCRNN | DMVSTNET``: train the predictor on the enhanced embedding of the frozen pretrained encoder (reference Run.py
    mode 'eval', model/Model.py:20-107, model/STGCN/args.py:52-88, model/TGCN/args.py:7-41, model/MTGNN/args.py:6-39, model/STSGCN/args.py:6-51, model/STFGNN/args.py:154-211, model/STGODE/args.py:10-178, model/MSDR/args.py:84-126, model/ST_WA/args.py:33-55, model/STMGCN_demand/args.py:7-56, model/CCRNN_demand/args.py:79-121 and model/DMVSTNET_demand/args.py:6-34 with the values of conf/<model>/<dataset>.conf)."""
    from types import SimpleNamespace
    from gptst_amd import graph
    from gptst_amd.enhance import EnhanceFrontEnd, xavier_downstream_
    from gptst_amd.eval_trainer import EvalTrainer
    from gptst_amd.predictors import ASTGCN, CCRNN, DMVSTNET, MSDR, MTGNN, STFGNN, STGCN, STGODE, STMGCN, STSGCN, STWA, TGCN
    if str(args.model) not in EVAL_MODELS:
        raise SystemExit("gpt-st_amd -mode eval implements -model STGCN, -model TGCN, -model MTGNN, -model ASTGCN, -model STSGCN, -model STFGNN, -model STGODE, -model MSDR, -model STWA, -model STMGCN, -model CCRNN and -model DMVSTNET (SURVEY.md §8f rank 4)")
    pargs = predictor_args(args.dataset, str(args.model), [a for a in sys.argv[1:] if a.startswith("--") or not a.startswith("-")])
    apply_predictor_overrides(args, pargs)       # reference Run.py:36-43: the predictor's schedule replaces the pretrain conf's (epochs 100, ...)
    if str(args.model) == "ASTGCN" and not args.xavier:
        raise SystemExit("-model ASTGCN needs --xavier True: its attention and Theta parameters are allocated uninitialised and only the xavier "
                         "pass gives them values (reference ASTGCN.py:55-59,98,137-141), so with xavier off the model has no defined initial state")
    init_seed(args.seed)
    args.log_dir = os.path.join(os.path.dirname(os.path.realpath(__file__)), "SAVE", args.dataset)
    os.makedirs(args.log_dir, exist_ok=True)
    data_root, (train, val, test, scaler, _, _) = load_series(args, dev)
    args.scaler_zeros = float(scaler.transform(0))
    csv_path = os.path.join(data_root, args.dataset, args.dataset + ".csv")
    A = (graph.adjacency_from_distance_csv(csv_path, args.num_nodes) if os.path.exists(csv_path)
         else graph.synthetic_adjacency(args.num_nodes, seed=args.seed))
    if str(args.model) == "TGCN":                                                # model/Model.py:67-69: built from the raw adjacency
        ap = SimpleNamespace(num_nodes=args.num_nodes, input_window=pargs.input_window, output_window=pargs.output_window,
                             rnn_units=pargs.rnn_units, output_dim=pargs.output_dim, G=graph.tgcn_graph(A))
        predictor = TGCN(ap, dev, args.hidden_dim, backend=str(args.tgcn_backend))
    elif str(args.model) == "MTGNN":                                             # model/Model.py:52-54: adj_mx feeds only predefined_A
        ap = SimpleNamespace(**vars(pargs), adj_mx=np.asarray(A, dtype=np.float32))
        predictor = MTGNN(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.mtgnn_backend))
    elif str(args.model) == "ASTGCN":                                            # ASTGCN.py:272-286: the polynomials of the raw adjacency
        ap = SimpleNamespace(**vars(pargs), G=graph.astgcn_graph(A, pargs.K))
        predictor = ASTGCN(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.astgcn_backend))
    elif str(args.model) == "STSGCN":                                            # model/Model.py:58-60, STSGCN/args.py:41-50: the raw adjacency
        ap = SimpleNamespace(**vars(pargs), A=np.asarray(A, dtype=np.float32))
        predictor = STSGCN(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.stsgcn_backend))
    elif str(args.model) == "STFGNN":                                            # model/Model.py, STFGNN/args.py:192-210: the fusion matrix
        ap = SimpleNamespace(**vars(pargs), adj=fusion_matrix(args, data_root, A, (train, val, test), scaler))
        predictor = STFGNN(ap, dev, args.hidden_dim, backend=str(args.stfgnn_backend))
    elif str(args.model) == "STGODE":                                            # model/Model.py, STGODE/args.py:176-177: the two normalised graphs
        sp, se = stgode_graphs(args, pargs, data_root, A, csv_path, train)
        ap = SimpleNamespace(**vars(pargs), A_sp_wave=sp, A_se_wave=se)
        predictor = STGODE(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.stgode_backend))
    elif str(args.model) == "MSDR":                                              # model/Model.py:79-82, MSDR/args.py:114-123: the raw adjacency
        ap = SimpleNamespace(**vars(pargs), supports=graph.msdr_supports(A, pargs.filter_type))
        predictor = MSDR(ap, dev, args.hidden_dim, backend=str(args.msdr_backend))
    elif str(args.model) == "STWA":                                              # model/Model.py:76-78: no graph (ST_WA.py:14 builds one nothing reads)
        predictor = STWA(SimpleNamespace(**vars(pargs)), dev, args.hidden_dim, backend=str(args.stwa_backend))
    elif str(args.model) == "STMGCN":                                            # model/Model.py, STMGCN_demand/args.py:35-53: the two support stacks
        dis, pcc = stmgcn_graphs(args, data_root, A, train)
        ap = SimpleNamespace(**vars(pargs), dis_graph=dis, pcc_graph=pcc)
        predictor = STMGCN(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.stmgcn_backend))
    elif str(args.model) == "CCRNN":                                             # model/Model.py:86-88, CCRNN_demand/args.py:112-120: the support
        ap = SimpleNamespace(**vars(pargs), support=ccrnn_support(args, pargs, data_root, (train, val, test), scaler))
        predictor = CCRNN(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.ccrnn_backend))
    elif str(args.model) == "DMVSTNET":                                          # model/Model.py, DMVSTNET_demand/args.py:32-33: the raw adjacency
        ap = SimpleNamespace(**vars(pargs), adj_mx=dmvstnet_adjacency(args, csv_path, A))
        predictor = DMVSTNET(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.dmvstnet_backend))
    else:
        ap = SimpleNamespace(Ks=pargs.Ks, Kt=pargs.Kt, num_nodes=args.num_nodes, G=graph.stgcn_graph(A), blocks1=list(pargs.blocks1),
                             drop_prob=pargs.drop_prob, outputl_ks=pargs.outputl_ks)
        predictor = STGCN(ap, dev, args.hidden_dim, args.output_dim, backend=str(args.stgcn_backend))
    model = EnhanceFrontEnd(args, predictor=predictor, finetune_encoder=bool(args.finetune_encoder)).to(dev)
    if args.xavier:                                                              # reference Run.py:79-85 (none of the other predictors' confs asks for it)
        xavier_downstream_(model)
    ckpt = args.log_dir + str(args.load_pretrain_path)                           # model/Model.py:92 (plain concatenation: '/GPTST_ada.pth')
    if os.path.exists(ckpt):
        model.load_pretrained_model(ckpt)                                        # model/Model.py:91-94
    elif "-demo_random_encoder" not in sys.argv and os.environ.get("GPTST_DEMO_RANDOM_ENCODER", "0") != "1":
        # the reference's load_pretrained_model raises on a missing file: "enhanced" results on a random frozen encoder are meaningless
        raise FileNotFoundError("no pretrained encoder at %s (run -mode pretrain first; -demo_random_encoder runs the plumbing on a "
                                "randomly initialised frozen encoder)" % ckpt)
    else:
        print("gpt-st_amd: no pretrained encoder at %s -> Xavier-initialised encoder (demo run)" % ckpt)
        for p_ in model.pretrain_model.parameters():                             # (all of them, the frozen ones too: xavier_init_ would skip those)
            torch.nn.init.xavier_uniform_(p_) if p_.dim() > 1 else torch.nn.init.uniform_(p_)
    EvalTrainer(model, args, train, val, test, float(scaler.mean), float(scaler.std)).train()


if __name__ == "__main__":
    main()
