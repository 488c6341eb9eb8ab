"""The models a trainer instantiates, assembled from the differentiable pieces: the reference's class names,
``forward`` signatures and parameter names (model/models.py), so that a trainer changes one import and a reference checkpoint loads.

    RobertaDot_NLL_LN                   roberta.embeddings.*, roberta.encoder.layer.N.*, embeddingHead.*, norm.*     -> [B, 768]
    RobertaDot_CLF_ANN_NLL_MultiChunk   the same tower; body_emb reshapes [B, C * 512] to [B * C, 512]               -> [B, C, 768]
    BiEncoder                           question_model.*, ctx_model.* under BertModel's names; no head               -> [B, H]
    SEEDEncoderDot_NLL_LN               seed_encoder.encoder.sentence_encoder.* under fairseq's names, embeddingHead.*, norm.*   -> [B, 768]

A tower is ``BertEmbeddings`` -> N - 1 x ``BertLayer.forward`` -> the last layer's ``forward_first_rows``: only h[:, 0] of the last
layer is ever read, so its query, output and feed-forward Linears and its seams run over the B first rows, and its attention is the
first-row core (``attention_first_row``).  There is one path; N = 1 is the last layer alone.  One tower call takes 1 + 3 N draws of
the dropout stream in the order embeddings, then per layer attention, first tail, second tail.  The head is ``F.linear`` +
``F.layer_norm`` (eps 1e-5), H -> 768 for both widths.  ``precision="half"`` is the form for ``torch.autocast``: the layers chain
through their 16-bit copies (BertLayer) and the residual stream stays fp32.  Lengths come from ``lens_from_mask``; nothing
synchronises, so a whole step can be captured.

``use_mean`` is not supported (no shipped recipe sets it).  An all-pad chunk of a MaxP document has length 0: the attention core
writes zeros for it, so its embedding is the tail of zeros -- finite, NOT the reference's value (which attends uniformly over the
pads) -- and it receives no gradient; ``nll_loss`` biases it by -9999 before the max, as the reference does, so it never wins.

Packed rows: ``model.set_packed_rows(query=Rq, body=Rb)`` makes the towers pack their padded ``[B, L]`` input
into R token rows (``ance_amd.packing``) and run every layer over those instead of B * L; ``None`` (the default) is the padded path
above, bit for bit; an int is a fixed capacity (what a captured step needs), ``"exact"`` reads the batch's total back and
synchronises.  ``forward``, ``query_emb`` and ``body_emb`` keep their signatures, and a tower call still takes 1 + 3 N draws in the
same order.  A sequence that does not fit the capacity is dropped: its embedding is NaN, and ``model.packed_dropped`` -- a 0-dim
int64 device tensor (created on the first packed call, not part of ``state_dict()``) that every packed tower call adds to -- counts
it.  MaxP packs its B * C chunks; an all-pad chunk is an EMPTY sequence there, whose embedding is the last layer's tails of a zero
residual and a zero context: finite, NOT the padded path's value (which is the tail of the pad token's hidden state), without a
gradient, and under the -9999 bias it never wins either.

Packed batches: every place that takes a tower's ``input_ids`` also takes a ``PackedTokens`` with
``attention_mask=None`` -- what ``TrainingBatches.packed(model)`` yields -- and runs the same packed tower on it as it is: no
``lens_from_mask``, no pack.  ``model.packed_dropped`` adds the batch's own count.  The batch must have been made under the tower's
rule (position mode, pad id, table sizes: ``tower.embeddings.pack_rule``); another rule is refused on the host.  MaxP reads its
chunk mask from ``seq_kept != 0``: a dropped chunk counts as present, so its NaN reaches the loss.

SEED-Encoder: the reference's tower masks every key whose id is the pad id, inside a record too, zeroes those
rows' embeddings and counts positions past them, so a pad row feeds nothing into a first row or a parameter gradient: leaving the
pad tokens out before the tower is exact.  ``SEEDEncoderDot_NLL_LN`` therefore has ONE path, the packed one: every call packs by id
(``pack_tokens_by_id``, three launches) into a capacity of B * L rows of that call -- under which nothing is dropped for capacity --
or what ``set_packed_rows`` says; ``attention_mask`` is accepted and ignored, as in the reference.  A sequence that BEGINS with the
pad id is dropped (NaN embedding, counted in ``packed_dropped``): its first row would not be its first token.  Not covered:
``PackedBatches`` / the device cursor for SEED (the padded ``TrainingBatches`` gather feeds the model), MaxP (the reference has no
SEED MaxP class), a non-zero activation_dropout.
"""
import collections

import torch

from . import _lib
from .attention import lens_from_mask
from .embeddings import BertEmbeddings, SeedEmbeddings
from .encoder import count_layers
from .layers import BertLayer, SeedLayer, _Names, _Namespace
from .loss import nll_loss
from .packing import PackedTokens

__all__ = ["TowerConfig", "RobertaDot_NLL_LN", "RobertaDot_CLF_ANN_NLL_MultiChunk", "BiEncoder", "SEEDEncoderDot_NLL_LN"]

OUT_DIM, HEAD_EPS = 768, 1e-5


class TowerConfig(object):
    """The attributes of a transformers config that a tower reads, under their names there; any object that has them will do."""

    def __init__(self, vocab_size, hidden_size, num_hidden_layers, intermediate_size, max_position_embeddings, type_vocab_size,
                 layer_norm_eps, pad_token_id, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, num_attention_heads=None):
        self.vocab_size, self.hidden_size, self.num_hidden_layers = int(vocab_size), int(hidden_size), int(num_hidden_layers)
        self.intermediate_size, self.max_position_embeddings = int(intermediate_size), int(max_position_embeddings)
        self.type_vocab_size, self.layer_norm_eps, self.pad_token_id = int(type_vocab_size), float(layer_norm_eps), int(pad_token_id)
        self.hidden_dropout_prob, self.attention_probs_dropout_prob = float(hidden_dropout_prob), float(attention_probs_dropout_prob)
        self.num_attention_heads = self.hidden_size // 64 if num_attention_heads is None else int(num_attention_heads)

    @classmethod
    def from_state_dict(cls, sd, prefix, roberta, dropout=0.1):
        """The shape of the tower under ``prefix``, inferred as ance_amd/encoder.py infers it; RoBERTa: eps 1e-5, pad id 1; BERT:
        eps 1e-12, pad id 0."""
        n = count_layers(sd, prefix)
        if n == 0:
            raise KeyError("no '%sencoder.layer.*' weights in state dict" % prefix)
        e = prefix + "embeddings."
        word, pos, types = (sd[e + k + "_embeddings.weight"] for k in ("word", "position", "token_type"))
        return cls(word.shape[0], word.shape[1], n, sd[prefix + "encoder.layer.0.intermediate.dense.weight"].shape[0], pos.shape[0],
                   types.shape[0], 1e-5 if roberta else 1e-12, 1 if roberta else 0, dropout, dropout)


class _Layers(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layer = torch.nn.ModuleList(layers)


def _check_packed_batch(embeddings, packed):
    want = embeddings.pack_rule
    if packed.rule != want:
        raise _lib.AnceLibraryError("the packed batch was made under %r, this tower's rule is %r" % (packed.rule, want))
    dev = embeddings.word_embeddings.weight.device
    if packed.ids.device != dev:
        raise _lib.AnceLibraryError("the packed batch is on %s, the tower on %s" % (packed.ids.device, dev))


def _chain_layers(h, layers, precision, step, last_step, where):
    """N - 1 layers and the last layer's first rows.  ``step(layer, h, where, ...)`` / ``last_step(layer, h, where, ...)`` are the
    layers' methods of the form, padded or packed, as plain functions; ``where`` is what they take behind the hidden states (lens,
    or the PackedTokens).  precision="half": chained through the 16-bit copy, one activation cast in the whole tower."""
    if precision == "half":
        h16 = None
        for layer in layers[:-1]:
            h, h16 = step(layer, h, where, hidden_states_half=h16, return_half=True)
        return last_step(layers[-1], h, where, hidden_states_half=h16)
    for layer in layers[:-1]:
        h = step(layer, h, where)
    return last_step(layers[-1], h, where)


def _run_packed_rows(embeddings, layers, precision, packed):
    """The embeddings, N - 1 layers and the last layer's first rows over the R rows of a PackedTokens."""
    return _chain_layers(embeddings.forward_packed(packed), layers, precision, BertLayer.forward_packed,
                         BertLayer.forward_first_rows_packed, packed)


class _Tower(torch.nn.Module):
    """embeddings.*, encoder.layer.N.* as BertModel / RobertaModel name them; ``forward`` returns the last layer's first rows."""

    def __init__(self, config, position_mode, precision):
        super().__init__()
        c = config
        if c.num_hidden_layers < 1:
            raise _lib.AnceLibraryError("a tower needs at least one layer")
        self.precision = precision
        self.embeddings = BertEmbeddings(c.vocab_size, c.hidden_size, c.max_position_embeddings, c.type_vocab_size, c.layer_norm_eps,
                                         c.hidden_dropout_prob, c.pad_token_id, position_mode)
        self.encoder = _Layers([BertLayer(c.hidden_size, c.num_attention_heads, c.intermediate_size, c.layer_norm_eps,
                                          c.hidden_dropout_prob, c.attention_probs_dropout_prob, precision=precision)
                                for _ in range(c.num_hidden_layers)])

    def _forward_packed(self, input_ids, lens, token_type_ids, rows, dropped):
        """The tower over R packed rows: pack (two launches, no draw), then ``_run_packed``."""
        return self._run_packed(self.embeddings.pack(input_ids, lens, rows, token_type_ids, dropped))

    def _check_packed(self, packed):
        _check_packed_batch(self.embeddings, packed)

    def _run_packed(self, packed):
        return _run_packed_rows(self.embeddings, self.encoder.layer, self.precision, packed)

    def forward(self, input_ids, attention_mask, token_type_ids=None, packed_rows=None, dropped=None):
        """packed_rows: None (the padded path), an int capacity or "exact"; dropped: the counter a packed call adds to.  A
        PackedTokens as input_ids (attention_mask None) is run as it is."""
        if isinstance(input_ids, PackedTokens):
            if attention_mask is not None or token_type_ids is not None:
                raise _lib.AnceLibraryError("a PackedTokens carries its lengths: attention_mask and token_type_ids must be None")
            self._check_packed(input_ids)
            return self._run_packed(input_ids)
        if attention_mask is None:
            raise _lib.AnceLibraryError("attention_mask is required: the lengths come from it")
        lens = lens_from_mask(attention_mask)
        if packed_rows is not None:
            return self._forward_packed(input_ids, lens, token_type_ids, packed_rows, dropped)
        return _chain_layers(self.embeddings(input_ids, token_type_ids), self.encoder.layer, self.precision, BertLayer.__call__,
                             BertLayer.forward_first_rows, lens)   # __call__: a layer's hooks run, as in layer(h, lens)


def _never_used(key):
    """The tensors the reference's classes carry but never use: the poolers, RobertaForSequenceClassification's classifier and the
    position_ids buffers of later transformers."""
    return ".pooler." in key or key.startswith("classifier.") or key.endswith(".position_ids")


def _check_packed_rows(rows, what):
    if rows is None or rows == "exact":
        return rows
    if isinstance(rows, bool) or not isinstance(rows, int) or rows < 1:
        raise _lib.AnceLibraryError("set_packed_rows: %s must be None, \"exact\" or an int capacity >= 1, got %r" % (what, rows))
    return rows


class _Checkpointed(torch.nn.Module):
    """Loading and re-emitting a reference checkpoint; the packed-rows setting of the towers."""

    _packed_rows = (None, None)
    packed_dropped = None
    _never_used = staticmethod(_never_used)

    def set_packed_rows(self, query=None, body=None):
        """The token-row capacity of the query tower's and of the body tower's calls: None (padded, the default), "exact" (the
        batch's total, read back: synchronises) or an int.  A body capacity counts the rows of ONE body_emb call (MaxP: of its
        B * C chunks).  Returns self."""
        self._packed_rows = (_check_packed_rows(query, "query"), _check_packed_rows(body, "body"))
        dev = next(self.parameters()).device
        if dev.type == "cuda":
            self._dropped_counter(dev)   # here, not inside a step: a captured step only adds
        return self

    def _dropped_counter(self, dev):
        if self.packed_dropped is None or self.packed_dropped.device != dev:   # a plain attribute: not in state_dict()
            self.packed_dropped = torch.zeros((), dtype=torch.int64, device=dev)
        return self.packed_dropped

    def towers(self):
        """(the query tower, the body tower)."""
        raise NotImplementedError

    def _tower_packed(self, tower, packed, attention_mask):
        """A PackedTokens through a tower as it is; the model's counter adds the batch's own count."""
        tower._check_packed(packed)   # before the counter moves
        out = tower(packed, attention_mask)
        self._dropped_counter(packed.ids.device).add_(packed.dropped)
        return out

    def _tower(self, tower, which, input_ids, attention_mask):
        if isinstance(input_ids, PackedTokens):
            return self._tower_packed(tower, input_ids, attention_mask)
        rows = self._packed_rows[which]
        if rows is None:
            return tower(input_ids, attention_mask)
        return tower(input_ids, attention_mask, packed_rows=rows, dropped=self._dropped_counter(input_ids.device))

    def load_reference_state_dict(self, sd):
        """Strict on every used name; the tensors the reference carries but never uses (``*.pooler.*``, ``classifier.*``,
        ``*.position_ids``) are set aside for ``reference_state_dict``; any other unknown key is refused."""
        used = set(self.state_dict().keys())
        unknown = [k for k in sd if k not in used and not self._never_used(k)]
        if unknown:
            raise KeyError("unexpected keys in state dict: %s ..." % unknown[:4])
        missing = [k for k in self.state_dict() if k not in sd]
        if missing:
            raise KeyError("missing weights: %s ..." % missing[:4])
        self.load_state_dict(collections.OrderedDict((k, torch.as_tensor(v)) for k, v in sd.items() if k in used), strict=True)
        self._set_aside = collections.OrderedDict((k, torch.as_tensor(v).detach().clone()) for k, v in sd.items() if k not in used)
        return self

    def reference_state_dict(self):
        """``state_dict()`` (detached) plus the set-aside tensors: a loaded checkpoint round-trips, and ``Encoder(...)`` builds from
        it with no renaming."""
        out = collections.OrderedDict((k, v.detach()) for k, v in self.state_dict().items())
        out.update(getattr(self, "_set_aside", {}))
        return out


class RobertaDot_NLL_LN(_Checkpointed):
    """model/models.py: RobertaDot_NLL_LN (FirstP): ``norm(embeddingHead(roberta(ids)[0][:, 0]))``, NLL over (query, positive,
    negative) triplets.  ``config``: a transformers RobertaConfig or a TowerConfig."""

    def __init__(self, config, model_argobj=None, precision="fp32"):
        super().__init__()
        if model_argobj is not None and getattr(model_argobj, "use_mean", False):
            raise _lib.AnceLibraryError("use_mean is not supported: the last layer computes the first rows only")
        self.use_mean = False
        self.roberta = _Tower(config, "roberta", precision)
        self.embeddingHead = torch.nn.Linear(config.hidden_size, OUT_DIM)
        self.norm = torch.nn.LayerNorm(OUT_DIM, eps=HEAD_EPS)

    @classmethod
    def from_state_dict(cls, sd, precision="fp32", dropout=0.1):
        model = cls(TowerConfig.from_state_dict(sd, "roberta.", True, dropout), precision=precision)
        return model.to(sd["embeddingHead.weight"].device).load_reference_state_dict(sd)

    def _head(self, first_rows):
        F = torch.nn.functional
        e = F.linear(first_rows, self.embeddingHead.weight, self.embeddingHead.bias)
        return F.layer_norm(e.float(), (OUT_DIM,), self.norm.weight, self.norm.bias, HEAD_EPS)

    def towers(self):
        return self.roberta, self.roberta

    def query_emb(self, input_ids, attention_mask=None):
        return self._head(self._tower(self.roberta, 0, input_ids, attention_mask))

    def body_emb(self, input_ids, attention_mask=None):
        return self._head(self._tower(self.roberta, 1, input_ids, attention_mask))

    def _loss(self, q, a, b, mask_a, mask_b):
        return nll_loss(q, a, b)

    def forward(self, query_ids, attention_mask_q=None, input_ids_a=None, attention_mask_a=None, input_ids_b=None, attention_mask_b=None,
                is_query=True):
        if input_ids_b is None and is_query:
            return self.query_emb(query_ids, attention_mask_q)
        if input_ids_b is None:
            return self.body_emb(query_ids, attention_mask_q)
        q = self.query_emb(query_ids, attention_mask_q)
        a = self.body_emb(input_ids_a, attention_mask_a)
        b = self.body_emb(input_ids_b, attention_mask_b)
        packed = isinstance(input_ids_a, PackedTokens)   # a packed batch is its own mask
        return (self._loss(q, a, b, input_ids_a if packed else attention_mask_a, input_ids_b if packed else attention_mask_b),)


class RobertaDot_CLF_ANN_NLL_MultiChunk(RobertaDot_NLL_LN):
    """model/models.py: RobertaDot_CLF_ANN_NLL_MultiChunk (MaxP): a document is C chunks of ``base_len`` = 512 tokens, its score the
    max over the chunks; an all-pad chunk is biased by -9999 (module docstring: its embedding is finite, not the reference's)."""

    def __init__(self, config, model_argobj=None, precision="fp32"):
        super().__init__(config, model_argobj, precision)
        self.base_len = 512

    def body_emb(self, input_ids, attention_mask=None):
        if isinstance(input_ids, PackedTokens):
            C = input_ids.chunks
            if input_ids.max_seq_len != self.base_len or input_ids.n_seq % C:
                raise _lib.AnceLibraryError("body_emb: a packed document batch must hold chunks of base_len = %d tokens, got %d"
                                            % (self.base_len, input_ids.max_seq_len))
            return self._head(self._tower(self.roberta, 1, input_ids, attention_mask)).reshape(-1, C, OUT_DIM)
        B, full = input_ids.shape
        C = full // self.base_len
        if C < 1 or C * self.base_len != full:
            raise _lib.AnceLibraryError("body_emb: the document length %d is not a multiple of base_len = %d" % (full, self.base_len))
        e = self._head(self._tower(self.roberta, 1, input_ids.reshape(B * C, full // C), attention_mask.reshape(B * C, full // C)))
        return e.reshape(B, C, OUT_DIM)

    @staticmethod
    def chunk_mask(attention_mask, n_chunks):
        """[B, C] fp32: the first attention-mask entry of every chunk, as NLL_MultiChunk.forward reads it.  Of a PackedTokens:
        ``seq_kept != 0`` -- the same values for kept chunks; a dropped chunk counts as present, so its NaN reaches the loss."""
        if isinstance(attention_mask, PackedTokens):
            return (attention_mask.seq_kept != 0).reshape(-1, n_chunks).float()
        return attention_mask.reshape(attention_mask.shape[0], n_chunks, -1)[:, :, 0].float()

    def _loss(self, q, a, b, mask_a, mask_b):
        C = a.shape[1]
        return nll_loss(q, a, b, self.chunk_mask(mask_a, C), self.chunk_mask(mask_b, C))


class BiEncoder(_Checkpointed):
    """model/models.py: BiEncoder (DPR): two BERT towers under BertModel's names (absolute positions, two token types, eps 1e-12),
    no head: an embedding is the last layer's first row.  ``forward`` with a negative returns ``(loss,)`` over the triplets; without
    one it returns ``(q_embs, a_embs)``, which the trainer feeds to ``ance_amd.loss.biencoder_nll_loss``.  ``config``: a transformers
    BertConfig or a TowerConfig, for both towers."""

    def __init__(self, config, precision="fp32"):
        super().__init__()
        self.question_model = _Tower(config, "absolute", precision)
        self.ctx_model = _Tower(config, "absolute", precision)

    @classmethod
    def from_state_dict(cls, sd, precision="fp32", dropout=0.1):
        model = cls(TowerConfig.from_state_dict(sd, "question_model.", False, dropout), precision=precision)
        return model.to(sd["question_model.embeddings.word_embeddings.weight"].device).load_reference_state_dict(sd)

    def towers(self):
        return self.question_model, self.ctx_model

    def query_emb(self, input_ids, attention_mask=None):
        return self._tower(self.question_model, 0, input_ids, attention_mask)

    def body_emb(self, input_ids, attention_mask=None):
        return self._tower(self.ctx_model, 1, input_ids, attention_mask)

    def forward(self, query_ids, attention_mask_q=None, input_ids_a=None, attention_mask_a=None, input_ids_b=None, attention_mask_b=None):
        q = self.query_emb(query_ids, attention_mask_q)
        a = self.body_emb(input_ids_a, attention_mask_a)
        if input_ids_b is None:
            return (q, a)
        b = self.body_emb(input_ids_b, attention_mask_b)
        return (nll_loss(q, a, b),)


class _SeedSentenceEncoder(SeedEmbeddings):
    """fairseq's TransformerSentenceEncoder as the SEED-Encoder configures it, under its names: embed_tokens, embed_positions,
    layers.N.*, emb_layer_norm (in the reference's order).  ``forward`` packs by id and returns the last layer's first rows."""

    def __init__(self, vocab_size, hidden_size, n_layers, n_heads, ffn_size, max_positions, padding_idx, dropout, attention_dropout,
                 precision):
        super().__init__(vocab_size, hidden_size, max_positions, padding_idx, HEAD_EPS, dropout)
        if n_layers < 1:
            raise _lib.AnceLibraryError("a tower needs at least one layer")
        self.precision = precision
        self.layers = torch.nn.ModuleList([SeedLayer(hidden_size, n_heads, ffn_size, HEAD_EPS, dropout, attention_dropout, precision)
                                           for _ in range(n_layers)])
        self._modules["emb_layer_norm"] = self._modules.pop("emb_layer_norm")   # after the layers, as the reference registers it

    def _check_packed(self, packed):
        _check_packed_batch(self, packed)

    def forward(self, input_ids, attention_mask=None, packed_rows=None, dropped=None):
        """input_ids [B, L] (packed by id into packed_rows rows, None: B * L) or a PackedTokens under the "seed" rule (run as it is);
        attention_mask is ignored: the keys are masked by id."""
        if isinstance(input_ids, PackedTokens):
            self._check_packed(input_ids)
            packed = input_ids
        else:
            if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.numel() == 0:
                raise _lib.AnceLibraryError("input_ids must be a CUDA(HIP) int32 or int64 tensor [B, L]")
            packed = self.pack(input_ids, input_ids.numel() if packed_rows is None else packed_rows, dropped)
        return _run_packed_rows(self, self.layers, self.precision, packed)


def _seed_never_used(key):
    return key.startswith("classification_heads.")


class SEEDEncoderDot_NLL_LN(RobertaDot_NLL_LN):
    """model/models.py: SEEDEncoderDot_NLL_LN: ``norm(embeddingHead(seed_encoder.encoder(ids)[:, 0]))`` over fairseq's post-LayerNorm
    sentence encoder, NLL over (query, positive, negative) triplets; body_emb is query_emb.  ``config``: the reference's
    SEEDEncoderConfig or any object with its attribute names (pad_token_id, vocab_size, encoder_layers, encoder_embed_dim,
    encoder_ffn_embed_dim, encoder_attention_heads, dropout, attention_dropout, activation_dropout, encoder_layerdrop,
    max_positions, activation_fn, quant_noise_pq).  The tower has one path, packed by id (module docstring).
    ``classification_heads.*``, which the reference carries and never uses, is set aside on loading and re-emitted."""

    _never_used = staticmethod(_seed_never_used)

    def __init__(self, config, model_argobj=None, precision="fp32"):
        _Checkpointed.__init__(self)
        c = config
        if model_argobj is not None and getattr(model_argobj, "use_mean", False):
            raise _lib.AnceLibraryError("use_mean is not supported: the last layer computes the first rows only")
        if float(getattr(c, "activation_dropout", 0.0)) != 0.0:
            raise _lib.AnceLibraryError("activation_dropout = %r is not supported: the GELU and fc2 are fused without a dropout between "
                                        "them (the shipped configs set 0.0)" % (c.activation_dropout,))
        if float(getattr(c, "encoder_layerdrop", 0.0)) != 0.0:
            raise _lib.AnceLibraryError("encoder_layerdrop = %r is not supported: every layer runs" % (c.encoder_layerdrop,))
        if float(getattr(c, "quant_noise_pq", 0.0)) != 0.0:
            raise _lib.AnceLibraryError("quant_noise_pq = %r is not supported" % (c.quant_noise_pq,))
        if getattr(c, "activation_fn", "gelu") != "gelu":
            raise _lib.AnceLibraryError("activation_fn = %r is not supported: the feed-forward seam is the erf GELU" % (c.activation_fn,))
        if (c.encoder_embed_dim, c.encoder_attention_heads, c.encoder_ffn_embed_dim) != (768, 12, 3072):
            raise _lib.AnceLibraryError("encoder_embed_dim = %r with %r heads and encoder_ffn_embed_dim = %r is not supported: the "
                                        "SEED-Encoder is 768 wide with 12 heads and a feed-forward width of 3072"
                                        % (c.encoder_embed_dim, c.encoder_attention_heads, c.encoder_ffn_embed_dim))
        self.use_mean = False
        self.seed_encoder = _Namespace()
        self.seed_encoder.encoder = _Namespace()
        self.seed_encoder.encoder.sentence_encoder = _SeedSentenceEncoder(
            int(c.vocab_size), int(c.encoder_embed_dim), int(c.encoder_layers), int(c.encoder_attention_heads),
            int(c.encoder_ffn_embed_dim), int(c.max_positions), int(c.pad_token_id), float(c.dropout), float(c.attention_dropout), precision)
        self.embeddingHead = torch.nn.Linear(c.encoder_embed_dim, OUT_DIM)
        self.norm = torch.nn.LayerNorm(OUT_DIM, eps=HEAD_EPS)

    @classmethod
    def from_state_dict(cls, sd, precision="fp32", dropout=0.1):
        """The shape of the tower from the weights themselves; pad id 1, as in the reference's config."""
        from .encoder import SEED_PREFIX
        word, pos = sd[SEED_PREFIX + "embed_tokens.weight"], sd[SEED_PREFIX + "embed_positions.weight"]
        n = 0
        while "%slayers.%d.fc1.weight" % (SEED_PREFIX, n) in sd:
            n += 1
        if n == 0:
            raise KeyError("no '%slayers.*' weights in state dict" % SEED_PREFIX)
        H, pad = int(word.shape[1]), 1
        config = _Names(pad_token_id=pad, vocab_size=int(word.shape[0]), encoder_layers=n, encoder_embed_dim=H,
                        encoder_ffn_embed_dim=int(sd[SEED_PREFIX + "layers.0.fc1.weight"].shape[0]), encoder_attention_heads=H // 64,
                        dropout=dropout, attention_dropout=dropout, activation_dropout=0.0, encoder_layerdrop=0.0,
                        max_positions=int(pos.shape[0]) - pad - 1, activation_fn="gelu", quant_noise_pq=0.0)
        model = cls(config, precision=precision)
        return model.to(sd["embeddingHead.weight"].device).load_reference_state_dict(sd)

    @property
    def sentence_encoder(self):
        return self.seed_encoder.encoder.sentence_encoder

    def towers(self):
        return self.sentence_encoder, self.sentence_encoder

    def _tower(self, tower, which, input_ids, attention_mask):
        if isinstance(input_ids, PackedTokens):
            return self._tower_packed(tower, input_ids, None)   # the mask is ignored: the keys are masked by id
        return tower(input_ids, None, packed_rows=self._packed_rows[which], dropped=self._dropped_counter(input_ids.device))

    def query_emb(self, input_ids, attention_mask=None):
        return self._head(self._tower(self.sentence_encoder, 0, input_ids, attention_mask))

    def body_emb(self, input_ids, attention_mask=None):
        return self._head(self._tower(self.sentence_encoder, 1, input_ids, attention_mask))
