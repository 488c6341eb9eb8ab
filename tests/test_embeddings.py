"""The trainable embeddings without a GPU.
Tests of the new library code (they fail without it): the C ABI's symbols, workspace query and refusals (host-side validation,
before any launch), the Python checks, the module's state-dict names.
Tests of the YARDSTICKS only -- tests/embeddings_util.py, which the GPU tests measure the kernels against; they run no library code
and would pass without it: the eager expression against the installed transformers modules bit for bit, the fp64 restatement
against autograd in float64 and against the reference's own tensors (tests/golden/embeddings*.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import embeddings_util as U
from ance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ance_embed_segment_chunk", "ance_embed_workspace_bytes", "ance_embed_forward", "ance_embed_backward")
CANARY = 0x7FC00ABC


def test_header_binding_and_library_export_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ance_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    L = _lib.lib()
    assert L.ance_abi_version() == 7                                  # symbols are only added
    assert L.ance_embed_segment_chunk() == _lib.EMBED_SEGMENT_CHUNK == int(re.search(r"#define ANCE_EMBED_SEGMENT_CHUNK (\d+)", src).group(1))
    for field, _ in _lib.AnceEmbedArgs._fields_ + _lib.AnceEmbedGradArgs._fields_:
        assert re.search(r"\b%s\b" % field, src), field


def test_workspace_query_is_pure():
    L = _lib.lib()
    R, C = _lib.LAYER_TAIL_ROWS_PER_WORKGROUP, _lib.EMBED_SEGMENT_CHUNK
    for H in (768, 1024):
        for T in (1, 15, 16, 17, 64, 65, 2085, 32768):
            S = 2 * ((4 * T + 255) // 256 * 256)
            want = S + T * H * 4 + -(-T // R) * 3 * H * 4 + 3 * -(-T // C) * 2 * H * 4   # the layout of include/ance_amd.h
            assert L.ance_embed_workspace_bytes(T, H) == want == L.ance_embed_workspace_bytes(T, H)
    for T, H in ((0, 768), (-1, 768), (1 << 31, 768), (16, 512), (16, 769), (16, 3072), (16, 0)):
        assert L.ance_embed_workspace_bytes(T, H) == 0, (T, H)


def _host_call(n_seq=3, L=8, H=768, vocab=100, max_pos=16, n_types=2):
    """Valid arguments over HOST memory (never dereferenced: every call below is refused before a launch); outputs hold a canary."""
    T = n_seq * L
    need = _lib.lib().ance_embed_workspace_bytes(T, H)
    f = lambda *shape: np.zeros(shape, np.float32)   # noqa: E731
    canary = lambda *shape: np.full(shape, CANARY, np.int32)   # noqa: E731
    ins = dict(ids=np.zeros((n_seq, L), np.int32), type_ids=np.zeros((n_seq, L), np.int32), word=f(vocab, H), pos=f(max_pos, H),
               type=f(n_types, H), gamma=f(H), beta=f(H), dy=f(T, H), keys=np.zeros(T, np.int32), perm=np.zeros(T, np.int64))
    outs = dict(y=canary(T, H), positions=canary(T), ws=canary(need // 4), dword=canary(vocab, H), dpos=canary(max_pos, H),
                dtype=canary(n_types, H), dgamma=canary(H), dbeta=canary(H))
    p = lambda a: a.ctypes.data   # noqa: E731
    a = _lib.AnceEmbedArgs(ids=p(ins["ids"]), type_ids=p(ins["type_ids"]), word=p(ins["word"]), pos=p(ins["pos"]), type=p(ins["type"]),
                           gamma=p(ins["gamma"]), beta=p(ins["beta"]), y=p(outs["y"]), positions=p(outs["positions"]), n_seq=n_seq, L=L, H=H,
                           vocab=vocab, max_pos=max_pos, n_types=n_types, position_mode=0, padding_idx=-1, eps=1e-5, dropout_p=0.1,
                           training=1, seed=1, offset=0, d_workspace=p(outs["ws"]), workspace_bytes=need)
    g = _lib.AnceEmbedGradArgs(dy=p(ins["dy"]), dword=p(outs["dword"]), dpos=p(outs["dpos"]), dtype=p(outs["dtype"]), dgamma=p(outs["dgamma"]),
                               dbeta=p(outs["dbeta"]), word_keys=p(ins["keys"]), word_perm=p(ins["perm"]), pos_keys=p(ins["keys"]),
                               pos_perm=p(ins["perm"]), type_keys=p(ins["keys"]), type_perm=p(ins["perm"]))
    return a, g, ins, outs, need


def _mutated(struct, kw):
    m = type(struct).from_buffer_copy(struct)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_refusals_happen_before_any_launch_and_leave_the_outputs_untouched():
    """Every refusal of include/ance_amd.h, on a box without a device: ANCE_E_INVALID with the entry point's name in
    ance_last_error, and no word of y, the saved buffers, the workspace or a gradient changes."""
    L = _lib.lib()
    a, g, ins, outs, need = _host_call()
    S = 2 * 256
    roberta = dict(position_mode=1, padding_idx=1)
    both = [dict(ids=None), dict(word=None), dict(pos=None), dict(type=None), dict(gamma=None), dict(d_workspace=None),
            dict(H=512), dict(H=3072), dict(H=0), dict(L=0), dict(L=513), dict(L=-1), dict(n_seq=0), dict(n_types=0), dict(n_types=3),
            dict(max_pos=7),                                   # absolute: L > max_pos
            dict(roberta, max_pos=9),                          # roberta: L + padding_idx + 1 = 10 > 9
            dict(roberta, positions=None), dict(position_mode=1, padding_idx=-1), dict(position_mode=2),
            dict(dropout_p=1.0), dict(dropout_p=-0.25), dict(dropout_p=float("nan")), dict(eps=0.0), dict(eps=-1e-5),
            dict(workspace_bytes=0), dict(word=a.word + 4), dict(gamma=a.gamma + 8), dict(d_workspace=a.d_workspace + 4)]
    fwd_only = [dict(y=None), dict(beta=None), dict(workspace_bytes=S - 1), dict(y=a.y + 4)]
    bwd_only = [dict(workspace_bytes=need - 1), dict(workspace_bytes=S)]
    bad_grads = [dict(dy=None), dict(dy=g.dy + 4), dict(dword=g.dword + 4), dict(dgamma=g.dgamma + 4), dict(word_keys=None), dict(word_perm=None),
                 dict(type_keys=None), dict(type_perm=None), dict(word_perm=g.word_perm + 4)]
    for kw in both + fwd_only:
        assert L.ance_embed_forward(ctypes.byref(_mutated(a, kw)), None) == -1, kw
        assert b"ance_embed_forward" in L.ance_last_error(), kw
    for kw in both + bwd_only:
        assert L.ance_embed_backward(ctypes.byref(_mutated(a, kw)), ctypes.byref(g), None) == -1, kw
        assert b"ance_embed_backward" in L.ance_last_error(), kw
    for kw in bad_grads:
        assert L.ance_embed_backward(ctypes.byref(a), ctypes.byref(_mutated(g, kw)), None) == -1, kw
    rob = _mutated(a, dict(roberta))
    for kw in (dict(pos_keys=None), dict(pos_perm=None)):   # roberta positions are grouped by a sort; absolute ones are not
        assert L.ance_embed_backward(ctypes.byref(rob), ctypes.byref(_mutated(g, kw)), None) == -1, kw
    assert L.ance_embed_forward(None, None) == -1 and L.ance_embed_backward(None, ctypes.byref(g), None) == -1
    assert L.ance_embed_backward(ctypes.byref(a), None, None) == -1
    for name, buf in outs.items():
        assert np.all(buf == CANARY), name
    # the text names the cause
    for kw, why in ((dict(H=512), b"768 or 1024"), (dict(L=513), b"L outside"), (dict(n_types=3), b"n_types"), (dict(max_pos=7), b"L > max_pos"),
                    (dict(roberta, max_pos=9), b"L + padding_idx + 1 > max_pos"), (dict(eps=0.0), b"eps"), (dict(dropout_p=1.0), b"dropout_p"),
                    (dict(workspace_bytes=0), b"workspace")):
        assert L.ance_embed_forward(ctypes.byref(_mutated(a, kw)), None) == -1 and why in L.ance_last_error(), (kw, L.ance_last_error())


def test_the_python_checks_raise_before_the_library_is_called():
    from ance_amd.embeddings import bert_embeddings
    w = torch.zeros(10, 768)
    with pytest.raises(_lib.AnceLibraryError, match="CUDA"):
        bert_embeddings(torch.zeros(1, 4, dtype=torch.int64), w, w, w[:2], w[0], w[0], 1e-5)
    with pytest.raises(_lib.AnceLibraryError, match="H in"):
        bert_embeddings(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(10, 512), w, w[:2], w[0], w[0], 1e-5)


# ---------------------------------------------------------------------------------------------------------------- the module
def _sub_dict(kind):
    from oracle import encoder_ref
    kw = dict(kind="bert", vocab=30522, max_pos=512, prefixes=("",)) if kind == "bert" else {}
    sd = encoder_ref.det_state_dict(seed=3, n_layers=0, head=False, ln_jitter=0.1, **kw)
    e = ("" if kind == "bert" else "roberta.") + "embeddings."
    return {k[len(e):]: v for k, v in sd.items() if k.startswith(e)}


@pytest.mark.parametrize("kind", ["roberta", "bert"])
def test_module_loads_both_towers_embeddings_strictly(kind):
    from ance_amd.embeddings import BertEmbeddings
    sd = _sub_dict(kind)
    assert sorted(sd) == sorted(U.PARAMS)
    if kind == "bert":
        m = BertEmbeddings(30522, 768, 512, 2, 1e-12, 0.1, pad_token_id=0)
    else:
        m = BertEmbeddings(50265, 768, 514, 1, 1e-5, 0.1, pad_token_id=1, position_mode="roberta")
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert sorted(m.state_dict().keys()) == sorted(U.PARAMS) == sorted(n for n, _ in m.named_parameters())
    assert torch.equal(m.word_embeddings.weight, sd["word_embeddings.weight"])
    bad = dict(sd, **{"position_embeddings.weight": sd["position_embeddings.weight"][:-1]})
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(bad, strict=True)
    with pytest.raises(RuntimeError, match="[Mm]issing"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "LayerNorm.bias"}, strict=True)


def test_module_refuses_what_the_kernels_do_not_have():
    from ance_amd.embeddings import BertEmbeddings
    for kw in (dict(hidden_size=512), dict(type_vocab_size=3), dict(position_mode="relative"), dict(position_mode="roberta", pad_token_id=None)):
        args = dict(dict(vocab_size=100, hidden_size=768, max_position_embeddings=64, type_vocab_size=2, pad_token_id=0), **kw)
        with pytest.raises(_lib.AnceLibraryError):
            BertEmbeddings(**args)


# ---------------------------------------------------------------------------------------------------------------- the utilities
# (from here on no library code runs: these pin the references of tests/test_gpu_embeddings.py)
def _ids_with_interior_pads(vocab, pad, B=5, L=12):
    ids = U.seeded_ids("cpu", (B, L), 3, vocab)
    ids[0, [2, 5, 6]] = pad          # interior pads
    ids[1, 7:] = pad                 # right padding
    ids[2, :] = pad                  # pads only
    ids[3, 0] = pad                  # a leading pad
    ids[4, 0], ids[4, 1] = 0, vocab - 1
    return ids


@pytest.mark.parametrize("kind", ["bert", "roberta"])
def test_eager_expression_is_the_installed_transformers_module_bit_for_bit(kind):
    """Pins the association (word + type) + position and the position rule: the util's expression against transformers'
    BertEmbeddings / RobertaEmbeddings forward in eval mode on the CPU, interior pads included."""
    from transformers import BertConfig, RobertaConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings as HFBert
    from transformers.models.roberta.modeling_roberta import RobertaEmbeddings as HFRoberta
    vocab, max_pos, H = 200, 40, 768
    if kind == "bert":
        n_types, pad, mode, eps = 2, 0, "absolute", 1e-12
        hf = HFBert(BertConfig(vocab_size=vocab, hidden_size=H, max_position_embeddings=max_pos, type_vocab_size=2, layer_norm_eps=eps, pad_token_id=0))
    else:
        n_types, pad, mode, eps = 1, 1, "roberta", 1e-5
        hf = HFRoberta(RobertaConfig(vocab_size=vocab, hidden_size=H, max_position_embeddings=max_pos, type_vocab_size=1, layer_norm_eps=eps,
                                     pad_token_id=1))
    word, pos, typ, gamma, beta = U.embed_inputs("hf." + kind, H, vocab, max_pos, n_types)
    hf.load_state_dict(dict(zip(U.PARAMS, (torch.from_numpy(t) for t in (word, pos, typ, gamma, beta)))), strict=True)
    hf.eval()
    ids = _ids_with_interior_pads(vocab, pad)
    types = (U.seeded_ids("cpu.tt", ids.shape, 0, 2) if kind == "bert" else None)
    if kind == "roberta":
        want_pos = hf.create_position_ids_from_input_ids(torch.from_numpy(ids), pad).numpy()
        got_pos = U.positions(ids, "roberta", pad)
        assert np.array_equal(got_pos, want_pos) and np.all(got_pos[2] == pad) and got_pos[0, 3] == pad + 3
    with torch.no_grad():
        want = hf(input_ids=torch.from_numpy(ids), token_type_ids=None if types is None else torch.from_numpy(types)).numpy()
    got = U.embed_eager_fp32(ids, types, word, pos, typ, gamma, beta, eps, None, mode, pad, backward=False)["y"]
    assert np.array_equal(got.view(np.int32), want.reshape(-1, H).view(np.int32))


def test_fp64_restatement_matches_autograd_in_float64_and_its_padding_rows_are_zero():
    """embed_fp64's hand-written backward against torch's autograd in float64 (F.embedding with padding_idx), with a mask."""
    H, vocab, max_pos, pad = 768, 50, 30, 1
    word, pos, typ, gamma, beta = U.embed_inputs("cpu64", H, vocab, max_pos, 2)
    ids = _ids_with_interior_pads(vocab, pad, L=10)
    types = U.seeded_ids("cpu64.tt", ids.shape, 0, 2)
    dy = U.embed_dy("cpu64", ids.size, H)
    keep = U.tail_keep_mask(0.5, 7, 2, ids.size, H)
    for mode in ("absolute", "roberta"):
        want = U.embed_fp64(ids, types, word, pos, typ, gamma, beta, 1e-5, dy, mode, pad, keep, 0.5)
        auto = U.embed_eager_fp32(ids, types, word, pos, typ, gamma, beta, 1e-5, dy, mode, pad, keep, 0.5, dtype="float64")
        assert np.array_equal(want["word_rows"], auto["word_rows"])
        for n in U.NAMES:
            assert np.abs(want[n] - auto[n]).max() <= 1e-12 * np.abs(want[n]).max(), (mode, n)
        assert np.all(want["dword"][want["word_rows"] == pad] == 0) and np.abs(dy[(ids == pad).reshape(-1)]).max() > 0
        assert np.all(want["dpos"][pad] == 0) == (mode == "roberta")


@pytest.mark.parametrize("case", U.GOLDEN_CASES)
def test_restatement_agrees_with_the_references_own_tensors(golden_dir, case):
    """The fp64 restatement on the committed fp32 inputs against the reference's committed fp32 results: within the bound that the
    reference's own fp32-to-fp64 distance sets (the generator asserted 1e-12 relative agreement with the fp64 run itself)."""
    m, t = U.load_golden(golden_dir, case)
    assert all(v <= 1e-12 for v in m["fp64_restatement_rel"].values()) and m["param_names"] == list(U.PARAMS)
    tables = U.golden_tables(m)
    L = m["L"]
    want = U.embed_fp64(t["ids"], t["types"], *tables, m["eps"], t["dy"], m["position_mode"], m["padding_idx"])
    assert np.array_equal(want["word_rows"], t["word_rows"]) and np.all(want["dpos"][L + 2:] == 0)
    want["dpos"] = want["dpos"][:L + 2]
    for n in U.NAMES:
        d = float(np.abs(want[n] - t[n]).max())
        b = U.bound(max(m["ref_err"][n], m["same_inputs"][n]), np.abs(want[n]).max())
        print("golden %s %-6s restatement vs the reference's fp32 %.3e  bound %.3e" % (case, n, d, b))
        assert d <= b, (n, d, b)
