"""Generates the large-tower (RoBERTa-large width: hidden 1024, 16 heads, FFN 4096) golden vectors under tests/golden/ by running
the REAL reference's RobertaDot_NLL_LN / RobertaDot_CLF_ANN_NLL_MultiChunk (model/models.py:137-199, imported through
oracle/ref_harness.py) in the build container:

    python tests/golden/make_golden_large.py            # everything
    python tests/golden/make_golden_large.py e2e        # one piece (encoders | e2e); the manifest keeps the other entries

Weights: ``oracle.encoder_ref.det_state_dict(hidden=1024, inter=4096, n_layers=24, ln_jitter=0.1)`` (their sha256 goes to
large_manifest.json).  Outputs: encoder_large24.npz, encoder_large24_L512.npz (FirstP body_emb, 24 layers), encoder_large_maxp.npz
(MaxP body_emb, 4 x 512, 24 layers), e2e_large.json (the reference's generate_new_ann on a toy set, 4 layers), and in the manifest,
per encoder fixture, the reference's own fp32 distance from an fp64 run of the same class (``model.double()``)."""
import copy
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import encoder_ref, ref_harness, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LARGE = dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096)


def large_weights(seed, n_layers):
    return encoder_ref.det_state_dict(seed=seed, hidden=1024, inter=4096, n_layers=n_layers, ln_jitter=0.1)


def build_large(kind, n_layers, sd):
    """The reference's own class at RoBERTa-large width (RobertaConfig(hidden_size=1024, num_attention_heads=16,
    intermediate_size=4096, num_hidden_layers=n_layers)), every weight loaded from ``sd``."""
    ref = ref_harness.load_reference()
    cfg = ref_harness.roberta_config(n_layers, **LARGE)
    torch.manual_seed(0)
    cls = ref.models.RobertaDot_NLL_LN if kind == "rdot_nll" else ref.models.RobertaDot_CLF_ANN_NLL_MultiChunk
    m = cls(cfg)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    bad = [k for k in missing if not (k.startswith("classifier.") or "pooler" in k or "position_ids" in k)]
    assert not bad and not unexpected, (bad, unexpected)
    m.eval()
    return m


def run_both(m, ids, mask):
    """body_emb in the reference's fp32 and, for the manifest, the same class in fp64: (fp32 output, max |fp32 - fp64|)."""
    with torch.no_grad():
        e32 = m.body_emb(ids, mask)
        m64 = copy.deepcopy(m).double()
        e64 = m64.body_emb(ids, mask)
    del m64
    return e32, float((e32.double() - e64).abs().max())


def golden_encoders():
    rng = np.random.default_rng(1024)
    out = {}
    # FirstP, L = 128: lengths at the 32 / 64 tile edges, plus a record with pad ids inside its length (RoBERTa positions skip them,
    # the attention mask does not)
    w = dict(seed=81, n_layers=24, ln_jitter=0.1)
    sd = large_weights(81, 24)
    m = build_large("rdot_nll", 24, sd)
    L = 128
    lens = np.array([1, 2, 33, 64, 65, 128, 100], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), L, lens.astype(np.int64))
    inner = rng.choice(np.arange(1, 99), size=12, replace=False)
    ids[6, inner] = synth.PAD
    t = torch.from_numpy(ids).long()
    emb, d64 = run_both(m, t, encoder_ref.mask_from_lengths(lens, L))
    out["large24"] = dict(gen="det", hidden=1024, inter=4096, checksum=encoder_ref.state_dict_sha256(sd), fp32_vs_fp64=d64, **w)
    np.savez_compressed(os.path.join(OUT, "encoder_large24.npz"), ids=ids, lens=lens, emb=emb.numpy())

    # FirstP, L = 512: the 256-key borders of the long-sequence attention (same weights)
    lens5 = np.array([1, 255, 256, 257, 511, 512], dtype=np.int32)
    ids5 = synth.make_records(rng, len(lens5), 512, lens5.astype(np.int64))
    emb5, d64 = run_both(m, torch.from_numpy(ids5).long(), encoder_ref.mask_from_lengths(lens5, 512))
    out["large24_L512"] = dict(gen="det", hidden=1024, inter=4096, checksum=encoder_ref.state_dict_sha256(sd), fp32_vs_fp64=d64, **w)
    np.savez_compressed(os.path.join(OUT, "encoder_large24_L512.npz"), ids=ids5, lens=lens5, emb=emb5.numpy())
    del m

    # MaxP, RobertaDot_CLF_ANN_NLL_MultiChunk.body_emb (model/models.py:165-199), 4 x 512: documents straddling the chunk borders,
    # all-pad chunks behind the short ones (same weights: the classes share every tower and head parameter)
    m2 = build_large("rdot_nll_multi_chunk", 24, sd)
    lens2 = np.array([2048, 1025, 513, 511, 40], dtype=np.int32)
    ids2 = synth.make_records(rng, len(lens2), 2048, lens2.astype(np.int64))
    emb2, d64 = run_both(m2, torch.from_numpy(ids2).long(), encoder_ref.mask_from_lengths(lens2, 2048))
    out["large_maxp"] = dict(gen="det", hidden=1024, inter=4096, checksum=encoder_ref.state_dict_sha256(sd), fp32_vs_fp64=d64, **w)
    np.savez_compressed(os.path.join(OUT, "encoder_large_maxp.npz"), ids=ids2, lens=lens2, emb=emb2.numpy())
    return out


def golden_end_to_end():
    """The reference's own generate_new_ann (SURVEY.md 8c recipe, G.load_model replaced by the model built here) with a 4-layer
    large-width RobertaDot_NLL_LN, --ann_measure_topk_mrr, random.seed(5); CPU."""
    tmp = tempfile.mkdtemp(prefix="ance_golden_large_")
    try:
        data = os.path.join(tmp, "data")
        dargs = dict(n_passages=400, n_train=60, n_dev=20, L=64, Lq=32, seed=80)
        synth.make_msmarco_like(data, **dargs)
        w = dict(seed=83, n_layers=4, ln_jitter=0.1)
        sd = large_weights(83, 4)
        m = build_large("rdot_nll", 4, sd)
        outd = os.path.join(tmp, "out")
        jargs = dict(max_seq_length=64, max_query_length=32, topk_training=40, negative_sample=6, ann_chunk_factor=2,
                     ann_measure_topk_mrr=True, model_type="rdot_nll")
        res = ref_harness.run_generate_new_ann(data, outd, m, output_num=0, checkpoint_path="/x/checkpoint-100/", step=100,
                                               seed=5, **jargs)
        with open(os.path.join(outd, "ann_training_data_0")) as f:
            lines = f.read()
        with open(os.path.join(outd, "ann_ndcg_0")) as f:
            nd = json.load(f)
        meta = dict(gen="det", hidden=1024, inter=4096, checksum=encoder_ref.state_dict_sha256(sd), **w)
        with open(os.path.join(OUT, "e2e_large.json"), "w") as f:
            json.dump(dict(weights=meta, data=dargs,
                           args=dict(seed=5, output_num=0, checkpoint_path="/x/checkpoint-100/", per_gpu_eval_batch_size=16, **jargs),
                           ann_training_data_0=lines, ann_ndcg_0=nd, result=[res[0], res[1]]), f)
        return dict(weights=meta, ndcg=nd["ndcg"], lines=lines.count("\n"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    path = os.path.join(OUT, "large_manifest.json")
    man = json.load(open(path)) if os.path.exists(path) else {}
    which = sys.argv[1:] or ["encoders", "e2e"]
    if "encoders" in which:
        man["encoder"] = golden_encoders()
    if "e2e" in which:
        man["e2e_large"] = golden_end_to_end()
    man.update(torch=torch.__version__, numpy=np.__version__)
    with open(path, "w") as f:
        json.dump(man, f, indent=1)
    print(json.dumps(man, indent=1))
