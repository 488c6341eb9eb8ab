"""Generates the SEED-Encoder golden vectors under tests/golden/ by running the REAL reference's SEEDEncoderDot_NLL_LN
(model/models.py:201-221, imported through oracle/ref_harness.py) in the build container:

    python tests/golden/make_golden_seed.py

Weights: ``oracle.encoder_ref.det_state_dict(kind="roberta", vocab=32769, max_pos=514)`` renamed to the reference's SEED names
(tests/seed_util.py); their sha256 goes to seed_manifest.json.  Outputs: encoder_seed12.npz, encoder_seed12_L512.npz (the
reference's body_emb, 12 layers) and e2e_seed.json (its generate_new_ann with model_type seeddot_nll on a toy set)."""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import encoder_ref, ref_harness, synth  # noqa: E402
from seed_util import SEED_VOCAB, det_seed_state_dict, interior_pads, into_seed_vocab, make_seed_msmarco_like  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def build_seed_model(n_layers, sd):
    """The reference's own SEEDEncoderDot_NLL_LN.  The installed transformers' init_weights needs attributes the reference's
    pretrained-model base never sets (all_tied_weights_keys): it is a no-op during construction -- every weight is loaded
    right after, strictly."""
    import transformers.modeling_utils as mu
    ref = ref_harness.load_reference()
    cfg = ref.models.MSMarcoConfigDict["seeddot_nll"].config_class(encoder_layers=n_layers)
    assert cfg.vocab_size == SEED_VOCAB and cfg.pad_token_id == 1 and cfg.max_positions == 512
    old = mu.PreTrainedModel.init_weights
    mu.PreTrainedModel.init_weights = lambda self: None
    try:
        m = ref.models.SEEDEncoderDot_NLL_LN(cfg)
    finally:
        mu.PreTrainedModel.init_weights = old
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("classification_heads.") for k in missing), missing
    m.eval()
    return m


def golden_encoders():
    rng = np.random.default_rng(4242)
    out = {}
    # L = 128: lengths at the 32 / 64 tile edges, records with pad ids inside their length, a [CLS] followed by pads only
    w = dict(seed=61, n_layers=12, ln_jitter=0.1)
    sd = det_seed_state_dict(**w)
    m = build_seed_model(12, sd)
    L = 128
    lens = np.array([1, 2, 33, 64, 65, 128, 40, 100, 128, 7], dtype=np.int64)
    ids = into_seed_vocab(synth.make_records(rng, len(lens), L, lens))
    ids[6:9] = interior_pads(rng, ids[6:9], lens[6:9], 0.2)
    ids[9, 1:] = synth.PAD  # [CLS] + pads inside the length
    with torch.no_grad():
        emb = m.body_emb(torch.from_numpy(ids).long(), None)
    out["seed12"] = dict(gen="det_seed", checksum=encoder_ref.state_dict_sha256(sd), **w)
    np.savez_compressed(os.path.join(OUT, "encoder_seed12.npz"), ids=ids, lens=lens.astype(np.int32), emb=emb.numpy())
    del m

    # L = 512: the 256-key borders of the long-sequence attention, and one record that crosses 256 only before compaction
    w = dict(seed=62, n_layers=12, ln_jitter=0.1)
    sd = det_seed_state_dict(**w)
    m = build_seed_model(12, sd)
    lens = np.array([1, 255, 256, 257, 511, 512, 300], dtype=np.int64)
    ids = into_seed_vocab(synth.make_records(rng, len(lens), 512, lens))
    ids[6:7] = interior_pads(rng, ids[6:7], lens[6:7], 0.25)
    with torch.no_grad():
        emb = m.body_emb(torch.from_numpy(ids).long(), None)
    out["seed12_L512"] = dict(gen="det_seed", checksum=encoder_ref.state_dict_sha256(sd), **w)
    np.savez_compressed(os.path.join(OUT, "encoder_seed12_L512.npz"), ids=ids, lens=lens.astype(np.int32), emb=emb.numpy())
    return out


def golden_end_to_end():
    """The reference's own generate_new_ann with model_type seeddot_nll (SURVEY.md 8c recipe, G.load_model replaced by the
    model built here), --ann_measure_topk_mrr, random.seed(5); CPU, 2 layers."""
    tmp = tempfile.mkdtemp(prefix="ance_golden_seed_")
    try:
        data = os.path.join(tmp, "data")
        dargs = dict(n_passages=400, n_train=60, n_dev=20, L=64, Lq=32, seed=78)
        make_seed_msmarco_like(data, pad_frac=0.05, **dargs)
        w = dict(seed=63, n_layers=2, ln_jitter=0.1)
        sd = det_seed_state_dict(**w)
        m = build_seed_model(2, sd)
        outd = os.path.join(tmp, "out")
        jargs = dict(max_seq_length=64, max_query_length=32, topk_training=40, negative_sample=6, ann_chunk_factor=2,
                     ann_measure_topk_mrr=True, model_type="seeddot_nll")
        res = ref_harness.run_generate_new_ann(data, outd, m, output_num=0, checkpoint_path="/x/checkpoint-100/", step=100,
                                               seed=5, **jargs)
        with open(os.path.join(outd, "ann_training_data_0")) as f:
            lines = f.read()
        with open(os.path.join(outd, "ann_ndcg_0")) as f:
            nd = json.load(f)
        meta = dict(gen="det_seed", checksum=encoder_ref.state_dict_sha256(sd), **w)
        with open(os.path.join(OUT, "e2e_seed.json"), "w") as f:
            json.dump(dict(weights=meta, data=dict(pad_frac=0.05, **dargs),
                           args=dict(seed=5, output_num=0, checkpoint_path="/x/checkpoint-100/", per_gpu_eval_batch_size=16, **jargs),
                           ann_training_data_0=lines, ann_ndcg_0=nd, result=[res[0], res[1]]), f)
        return dict(e2e_seed=dict(weights=meta, ndcg=nd["ndcg"], lines=lines.count("\n")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    man = dict(encoder=golden_encoders(), torch=torch.__version__, numpy=np.__version__)
    man.update(golden_end_to_end())
    with open(os.path.join(OUT, "seed_manifest.json"), "w") as f:
        json.dump(man, f, indent=1)
    print(json.dumps(man, indent=1))
