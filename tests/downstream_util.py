"""What the GPU tests of the four HIP predictors share (test_gpu_stgcn_hip.py, test_gpu_tgcn_hip.py, test_gpu_mtgnn_hip.py,
test_gpu_astgcn_hip.py): the error measure against an fp64 reference and its bound."""
TOL = 1e-4


def _err(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30))


def _check(parity, errs):
    for k, v in errs.items():
        parity(k, v)
    if len(errs) > 12:                                                   # a whole model's gradients: the worst one says it
        worst = max(errs, key=errs.get)
        print("worst of %d: %s %.2e" % (len(errs), worst, errs[worst]))
    else:
        print({k: "%.2e" % v for k, v in errs.items()})
    over = {k: v for k, v in errs.items() if not v < TOL}
    assert not over, over
