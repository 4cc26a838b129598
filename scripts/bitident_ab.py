"""Bit-identity check of an A/B build against the product library, with fixed inputs; --out saves
every output tensor (torch.save of this script's own tensors), --compare A B reports the tensors
that differ.  Default: the bf16 stack forward + backward at a rank shape (c4: B = 80, T = 160),
under --schedule (auto | per_step | per_layer | persist, passed to both), so the case can be saved
once per schedule.
--ge2e: the GE2E loss kernels on every case of tests/ge2e_cases.py and tests/contrast_cases.py, both
losses: the fused step, the split forward and backward (with GLOSS on its case), the sharded
three-call forms (fused and split) on the tables' shard lists, and the stand-alone helper ops with
their backward passes; saves loss, per, dE, dwdb and every shard's reduce buffer.
Usage: python scripts/bitident_ab.py [--ge2e | --schedule S] [--lib L] --out f.pt ; python scripts/bitident_ab.py --compare a.pt b.pt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--compare", nargs=2, default=None)
ap.add_argument("--B", type=int, default=80)
ap.add_argument("--T", type=int, default=160)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ge2e", action="store_true")
ap.add_argument("--schedule", default="auto", choices=["auto", "per_step", "per_layer", "persist"])
args = ap.parse_args()
if args.compare:
    a, b = (torch.load(f, weights_only=True) for f in args.compare)
    bad = [k for k in a if k not in b or not torch.equal(a[k], b[k])] + [k for k in b if k not in a]
    print({"tensors": len(a), "differ": bad})
    sys.exit(1 if bad else 0)
from pytorch_speaker_verification_amd import _lib  # noqa: E402
if args.lib:
    _lib.use_library(args.lib)
from pytorch_speaker_verification_amd import ops  # noqa: E402


def ge2e_outputs(dev):
    """{name: tensor} of every GE2E path on the tests' case tables (their inputs, read-only)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import contrast_cases as cc  # noqa: E402
    import ge2e_cases as gc  # noqa: E402
    from pytorch_speaker_verification_amd import utils  # noqa: E402
    from pytorch_speaker_verification_amd.sharded_ge2e import HipFusedShard, HipShardKernels  # noqa: E402
    out = {}

    def put(tag, **ts):
        for k, v in ts.items():
            out[f"{tag}.{k}"] = torch.as_tensor(v).detach().clone().cpu()

    def scal(v):
        return torch.tensor(v, dtype=torch.float32, device=dev)

    for method, tab in (("softmax", gc), ("contrast", cc)):
        cases = gc.FUSED_CASES + gc.SPLIT_CASES + ([cc.BIG_CASE] if method == "contrast" else [])
        for case in cases:
            N, M, D, w, b = case
            E, wt, bt = torch.tensor(tab.inputs(N, M, D), device=dev), scal(w), scal(b)
            tag = f"{method}.{gc.case_id(case)}"
            loss, per, dE, dwdb = ops.ge2e_train(E, wt, bt, loss_method=method)
            put(tag + ".train", loss=loss, per=per, dE=dE, dwdb=dwdb)
            for g in (None, gc.GLOSS) if case == gc.GLOSS_CASE else (None,):
                loss, per, st = ops.ge2e_forward(E, wt, bt, method)
                dE, dw, db = ops.ge2e_backward(st, wt, bt, None if g is None else scal(g))
                put(tag + f".split.g{g}", loss=loss, per=per, dE=dE, dw=dw, db=db)
        for kern, table in ((HipFusedShard, gc.SHARDED_CASES), (HipShardKernels, gc.SPLIT_SHARDED_CASES)):
            for (N, M, D), shards in table:
                k, wt, bt = kern(method), scal(gc.SHARD_W), scal(gc.SHARD_B)
                Et = torch.tensor(tab.inputs(N, M, D), device=dev)
                sl = gc.shard_slices(shards)
                parts = [Et[s0:s0 + nl].contiguous() for s0, nl in sl]
                tag = f"{method}.{kern.__name__}.{N}-{M}-{D}." + "+".join(map(str, shards))
                if kern is HipFusedShard:
                    prep = [k.prep(p, N) for p in parts]
                    ssum = torch.cat([p[0] for p in prep])
                    rows = [k.rows(p, s0, N, ssum, wt, bt, ws) for p, (s0, _), (_, ws) in zip(parts, sl, prep)]
                    red = torch.stack([r[2] for r in rows]).sum(0)
                    dEs = [k.finalize(p, s0, N, red.clone(), ws) for p, (s0, _), (_, ws) in zip(parts, sl, prep)]
                    for i, (r, dE) in enumerate(zip(rows, dEs)):
                        put(f"{tag}.shard{i}", ssum=prep[i][0], loss=r[0], per=r[1], red=r[2], dwdb=r[3], dE=dE)
                else:
                    ssum = torch.cat([k.speaker_sums(p) for p in parts])
                    fwd = [k.fwd_rows(p, s0, N, ssum, wt, bt) for p, (s0, _) in zip(parts, sl)]
                    bwd = [k.bwd_rows(f[2], wt, bt, None) for f in fwd]
                    red = torch.stack([r[0] for r in bwd]).sum(0)
                    for i, (f, r) in enumerate(zip(fwd, bwd)):
                        put(f"{tag}.shard{i}", loss=f[0], per=f[1], red=r[0], dwdb=r[1], dE=k.finalize(f[2], red.clone()))
    # the stand-alone helpers and their backward passes
    for N, M, D, Nc in gc.HELPER_CASES + [(5, 3, 64, 5)]:
        En, Eenr = gc.helper_inputs(N, M, D, Nc)
        E = torch.tensor(En, device=dev, requires_grad=True)
        Ee = torch.tensor(Eenr, device=dev, requires_grad=True)
        tag = f"helper.{N}-{M}-{D}-{Nc}"
        C = utils.get_centroids(Ee)
        put(tag, C=C)
        if Nc < N:
            continue
        cos = utils.get_cossim(E, C)
        S = 10.0 * cos - 5.0
        wts = torch.randn(N, M, generator=torch.Generator().manual_seed(78)).to(dev)
        for name, fn in (("calc_loss", utils.calc_loss), ("calc_loss_contrast", utils.calc_loss_contrast)):
            E.grad = Ee.grad = None
            loss, per = fn(S)
            (loss + (per * wts).sum()).backward(retain_graph=True)
            put(f"{tag}.{name}", cos=cos, loss=loss, per=per, dE=E.grad, dEenr=Ee.grad)
    return out


if args.ge2e:
    out = ge2e_outputs(torch.device("cuda", 0))
    again = ge2e_outputs(torch.device("cuda", 0))  # every launch must give the same bits
    assert all(torch.equal(out[k], again[k]) for k in out), "repeat differs"
    print({"tensors": len(out)})
    if args.out:
        torch.save(out, args.out)
    sys.exit(0)
from pytorch_speaker_verification_amd._lib import PersistStatus  # noqa: E402
from pytorch_speaker_verification_amd.speech_embedder_net import SpeechEmbedder  # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(0)
net = SpeechEmbedder().to(dev)
x = torch.randn(args.B, args.T, 40, device=dev)
layers = net.LSTM_stack.layer_params()
wp, bp = net.projection.weight, net.projection.bias
ps = PersistStatus(dev)
out = {}
for r in range(args.reps):  # repeated: every launch must give the same bits
    emb, st = ops.embedder_forward_bf16(x, layers, wp, bp, save=True, status=ps, schedule=args.schedule)
    demb = torch.randn(emb.shape, generator=torch.Generator(device=dev).manual_seed(7), device=dev) * 0.1
    grads = ops.embedder_backward_bf16(st, demb, layers, wp, status=ps, schedule=args.schedule)
    torch.cuda.synchronize()
    flat = {"emb": emb}
    for i, g in enumerate(grads if isinstance(grads, (list, tuple)) else [grads]):
        if isinstance(g, torch.Tensor):
            flat[f"g{i}"] = g
        elif isinstance(g, (list, tuple)):
            for j, h in enumerate(g):
                if isinstance(h, torch.Tensor):
                    flat[f"g{i}_{j}"] = h
    flat = {k: v.detach().clone().cpu() for k, v in flat.items()}
    if r == 0:
        out = flat
    else:
        assert all(torch.equal(out[k], flat[k]) for k in out), "repeat differs"
print({"status": int(ps.block[0]), "tensors": len(out)})
if args.out:
    torch.save(out, args.out)
