"""The input end of a trainable tower, differentiable (csrc/embed_train.hip behind ance_embed_*).

    y = bert_embeddings(input_ids, word, position, token_type, LayerNorm.weight, LayerNorm.bias, eps, token_type_ids,
                        position_mode, padding_idx, dropout_p, self.training)

is what transformers' eager ``BertEmbeddings.forward`` (``position_mode="absolute"``) and ``RobertaEmbeddings.forward``
(``"roberta"``: positions counted from the non-pad ids, pads anywhere in the row) compute --
``dropout(LayerNorm((word[ids] + token_type[types]) + position[p]))`` -- in one launch.  It keeps two floats per token (mean,
1 / sqrt(var + eps)) and, in roberta mode, the int32 positions; no mask and no [T, H] activation.  The backward recomputes the sum
from the tables, regenerates the mask and returns DENSE gradients for the three tables and the LayerNorm: a table gradient is a
segmented sum over the rows in the order of a stable device sort of the ids (``torch.sort(stable=True)``: the only torch kernels on
the path), without atomics -- the same inputs give the same bits (include/ance_amd.h states the order).  The row ``padding_idx`` of
the word table and, in roberta mode, of the position table gets a zero gradient, as ``nn.Embedding(padding_idx=...)`` gives it.

Ids outside a table are CLAMPED into it by the kernels (forward bits and gradient row of the nearest valid id); nothing is raised,
because finding out would mean a synchronisation.  Dropout draws from ``ance_amd.attention.dropout_state`` as every other dropout
of this package does; a call with ``training`` false or ``dropout_p == 0`` draws nothing.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .attention import _NO_DRAW, _custom_bwd, _custom_fwd, dropout_state
from .layers import TAIL_WIDTHS, _check_vector, _ptr, _stats_floats, _vector
from .packing import PackedTokens, PackRule

__all__ = ["bert_embeddings", "bert_embeddings_packed", "BertEmbeddings", "SeedEmbeddings"]

MAX_SEQ_LEN = 512


def _table(t):
    """A [n, H] table as the kernels read it: contiguous and 16-byte aligned."""
    t = t.detach()
    return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _ids32(t):
    return t.to(torch.int32).contiguous()


def _sorted(keys):
    """The grouping of include/ance_amd.h: (the keys in stable ascending order, the permutation), on the device."""
    return torch.sort(keys.view(-1), stable=True)


class _BertEmbeddings(torch.autograd.Function):
    @staticmethod
    @_custom_fwd
    def forward(ctx, word, position, token_type, weight, beta, input_ids, token_type_ids, eps, mode, padding_idx, dropout_p, training):
        L = _lib.lib()
        word, position, token_type = _table(word), _table(position), _table(token_type)
        weight, beta = _vector(weight), _vector(beta)
        n_seq, seq_len = input_ids.shape
        H, n_rows, dev = word.shape[1], n_seq * seq_len, word.device
        if L.ance_embed_workspace_bytes(n_rows, H) == 0:
            raise _lib.AnceLibraryError("bert_embeddings: unsupported shape (rows %d, width %d)" % (n_rows, H))
        ids = _ids32(input_ids)
        types = _ids32(token_type_ids) if token_type_ids is not None else None
        y = torch.empty((n_seq, seq_len, H), dtype=torch.float32, device=dev)
        stats = torch.empty(_stats_floats(n_rows), dtype=torch.float32, device=dev)
        positions = torch.empty(n_rows, dtype=torch.int32, device=dev) if mode == 1 else None
        drop = bool(training) and dropout_p > 0.0
        draw = dropout_state.draw(dev) if drop else _NO_DRAW
        args = _lib.AnceEmbedArgs(ids=ids.data_ptr(), type_ids=_ptr(types), word=word.data_ptr(), pos=position.data_ptr(),
                                  type=token_type.data_ptr(), gamma=weight.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(),
                                  positions=_ptr(positions), n_seq=n_seq, L=seq_len, H=H, vocab=word.shape[0],
                                  max_pos=position.shape[0], n_types=token_type.shape[0], position_mode=mode, padding_idx=padding_idx,
                                  eps=float(eps), dropout_p=float(dropout_p), training=1 if drop else 0, seed=draw.seed,
                                  offset=draw.offset, d_workspace=stats.data_ptr(), workspace_bytes=stats.numel() * 4)
        with torch.cuda.device(dev):
            draw.launch("ance_embed_forward", ctypes.byref(args))
        ctx.save_for_backward(word, position, token_type, weight, ids, types, positions, stats)
        ctx.args, ctx.draw = args, draw
        return y

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dy):
        L = _lib.lib()
        word, position, token_type, weight, ids, types, positions, stats = ctx.saved_tensors
        a = _lib.AnceEmbedArgs.from_buffer_copy(ctx.args)  # y and beta are not touched by the backward
        H, n_rows, dev = a.H, a.n_seq * a.L, word.device
        dy = dy.to(torch.float32).contiguous()
        if dy.data_ptr() % 16:
            dy = dy.clone()
        want_word, want_pos, want_type, want_w, want_b = ctx.needs_input_grad[:5]

        def table(want, like):  # dense and zero-filled: the kernels store the rows that occur
            return torch.zeros(like.shape, dtype=torch.float32, device=dev) if want else None

        dword, dpos, dtype = table(want_word, word), table(want_pos, position), table(want_type, token_type)
        dgamma = torch.empty(H, dtype=torch.float32, device=dev) if want_w else None
        dbeta = torch.empty(H, dtype=torch.float32, device=dev) if want_b else None
        # the saved state is the statistics (and the positions); the backward's rows and partial rows live only as long as this call
        ws_bytes = L.ance_embed_workspace_bytes(n_rows, H)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        ws[:stats.numel()].copy_(stats)
        a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        none = (None, None)
        wk, wp = _sorted(ids) if want_word else none
        pk, pp = _sorted(positions) if want_pos and positions is not None else none
        tk, tp = _sorted(types) if want_type and types is not None and a.n_types == 2 else none
        g = _lib.AnceEmbedGradArgs(dy=dy.data_ptr(), dword=_ptr(dword), dpos=_ptr(dpos), dtype=_ptr(dtype), dgamma=_ptr(dgamma),
                                   dbeta=_ptr(dbeta), word_keys=_ptr(wk), word_perm=_ptr(wp), pos_keys=_ptr(pk), pos_perm=_ptr(pp),
                                   type_keys=_ptr(tk), type_perm=_ptr(tp))
        with torch.cuda.device(dev):
            ctx.draw.launch("ance_embed_backward", ctypes.byref(a), ctypes.byref(g))
        return dword, dpos, dtype, dgamma, dbeta, None, None, None, None, None, None, None


class _BertEmbeddingsRows(torch.autograd.Function):
    """_BertEmbeddings over R packed rows whose positions are given (ance_embed_rows_*): ids, types, positions int32 [R]."""

    @staticmethod
    @_custom_fwd
    def forward(ctx, word, position, token_type, weight, beta, ids, types, positions, eps, mode, padding_idx, dropout_p, training):
        L = _lib.lib()
        word, position, token_type = _table(word), _table(position), _table(token_type)
        weight, beta = _vector(weight), _vector(beta)
        H, n_rows, dev = word.shape[1], ids.numel(), word.device
        if L.ance_embed_workspace_bytes(n_rows, H) == 0:
            raise _lib.AnceLibraryError("bert_embeddings_packed: unsupported shape (rows %d, width %d)" % (n_rows, H))
        y = torch.empty((n_rows, H), dtype=torch.float32, device=dev)
        stats = torch.empty(_stats_floats(n_rows), dtype=torch.float32, device=dev)
        drop = bool(training) and dropout_p > 0.0
        draw = dropout_state.draw(dev) if drop else _NO_DRAW
        args = _lib.AnceEmbedArgs(ids=ids.data_ptr(), type_ids=_ptr(types), word=word.data_ptr(), pos=position.data_ptr(),
                                  type=token_type.data_ptr(), gamma=weight.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(),
                                  positions=positions.data_ptr(), n_seq=n_rows, L=1, H=H, vocab=word.shape[0],
                                  max_pos=position.shape[0], n_types=token_type.shape[0], position_mode=mode, padding_idx=padding_idx,
                                  eps=float(eps), dropout_p=float(dropout_p), training=1 if drop else 0, seed=draw.seed,
                                  offset=draw.offset, d_workspace=stats.data_ptr(), workspace_bytes=stats.numel() * 4)
        with torch.cuda.device(dev):
            draw.launch("ance_embed_rows_forward", ctypes.byref(args))
        ctx.save_for_backward(word, position, token_type, weight, ids, types, positions, stats)
        ctx.args, ctx.draw = args, draw
        return y

    @staticmethod
    @_custom_bwd
    @once_differentiable
    def backward(ctx, dy):
        L = _lib.lib()
        word, position, token_type, weight, ids, types, positions, stats = ctx.saved_tensors
        a = _lib.AnceEmbedArgs.from_buffer_copy(ctx.args)  # y and beta are not touched by the backward
        H, n_rows, dev = a.H, a.n_seq, word.device
        dy = dy.to(torch.float32).contiguous()
        if dy.data_ptr() % 16:
            dy = dy.clone()
        want_word, want_pos, want_type, want_w, want_b = ctx.needs_input_grad[:5]

        def table(want, like):  # dense and zero-filled: the kernels store the rows that occur
            return torch.zeros(like.shape, dtype=torch.float32, device=dev) if want else None

        dword, dpos, dtype = table(want_word, word), table(want_pos, position), table(want_type, token_type)
        dgamma = torch.empty(H, dtype=torch.float32, device=dev) if want_w else None
        dbeta = torch.empty(H, dtype=torch.float32, device=dev) if want_b else None
        ws_bytes = L.ance_embed_workspace_bytes(n_rows, H)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        ws[:stats.numel()].copy_(stats)
        a.d_workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        none = (None, None)
        wk, wp = _sorted(ids) if want_word else none
        pk, pp = _sorted(positions) if want_pos else none   # in absolute mode too: a packed row is not s * L + p
        tk, tp = _sorted(types) if want_type and types is not None and a.n_types == 2 else none
        g = _lib.AnceEmbedGradArgs(dy=dy.data_ptr(), dword=_ptr(dword), dpos=_ptr(dpos), dtype=_ptr(dtype), dgamma=_ptr(dgamma),
                                   dbeta=_ptr(dbeta), word_keys=_ptr(wk), word_perm=_ptr(wp), pos_keys=_ptr(pk), pos_perm=_ptr(pp),
                                   type_keys=_ptr(tk), type_perm=_ptr(tp))
        with torch.cuda.device(dev):
            ctx.draw.launch("ance_embed_rows_backward", ctypes.byref(a), ctypes.byref(g))
        return dword, dpos, dtype, dgamma, dbeta, None, None, None, None, None, None, None, None


def _check_table(t, what, H, like=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.shape[0] < 1:
        raise _lib.AnceLibraryError("%s must be a CUDA(HIP) tensor [n, H]" % what)
    if t.dtype != torch.float32 and not (torch.is_autocast_enabled() and t.is_floating_point()):  # autocast: cast by _custom_fwd
        raise _lib.AnceLibraryError("%s must have dtype torch.float32, got %s" % (what, t.dtype))
    if t.shape[1] != H or (like is not None and t.device != like.device):
        raise _lib.AnceLibraryError("%s must be [n, %d] on the word table's device, got %r on %s" % (what, H, tuple(t.shape), t.device))


def _check_ids(t, what, like, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != like.device:
        raise _lib.AnceLibraryError("%s must be a CUDA(HIP) tensor on %s" % (what, like.device))
    if t.dtype not in (torch.int32, torch.int64):
        raise _lib.AnceLibraryError("%s must have dtype torch.int32 or torch.int64, got %s" % (what, t.dtype))
    if t.dim() != 2 or t.numel() == 0 or (shape is not None and t.shape != shape):
        raise _lib.AnceLibraryError("%s must be [B, L]%s, got %r" % (what, "" if shape is None else " like input_ids", tuple(t.shape)))


def bert_embeddings(input_ids, word, position, token_type, ln_weight, ln_bias, eps, token_type_ids=None, position_mode="absolute",
                    padding_idx=None, dropout_p=0.0, training=True):
    """dropout(LayerNorm((word[input_ids] + token_type[token_type_ids]) + position[p]) * ln_weight + ln_bias) -> [B, L, H] fp32.
    input_ids [B, L] int32 or int64 (L <= 512), token_type_ids like it or None (type 0); word [vocab, H], position [max_pos, H],
    token_type [1 or 2, H] fp32 with H 768 or 1024.  position_mode "absolute": p = the column, L <= max_pos; "roberta": p =
    padding_idx + the running count of non-pad ids (padding_idx at pads), L + padding_idx + 1 <= max_pos.  padding_idx (None: no
    such row; required in roberta mode) names the row of the word table -- and in roberta mode of the position table -- whose
    gradient stays zero.  Ids outside their table are clamped into it.  Gradients for the five parameters, the tables' dense."""
    if not isinstance(word, torch.Tensor) or word.dim() != 2 or word.shape[1] not in TAIL_WIDTHS:
        raise _lib.AnceLibraryError("word must be [vocab, H] with H in %r" % (TAIL_WIDTHS,))
    H = word.shape[1]
    _check_table(word, "word", H)
    _check_table(position, "position", H, word)
    _check_table(token_type, "token_type", H, word)
    _check_vector(ln_weight, "ln_weight", H, word)
    _check_vector(ln_bias, "ln_bias", H, word)
    _check_ids(input_ids, "input_ids", word)
    if token_type_ids is not None:
        _check_ids(token_type_ids, "token_type_ids", word, input_ids.shape)
    if position_mode not in _lib.EMBED_POSITION_MODES:
        raise _lib.AnceLibraryError("position_mode must be \"absolute\" or \"roberta\", got %r" % (position_mode,))
    seq_len, vocab, max_pos = input_ids.shape[1], word.shape[0], position.shape[0]
    pad = -1 if padding_idx is None else int(padding_idx)
    if seq_len > MAX_SEQ_LEN:
        raise _lib.AnceLibraryError("input_ids: L = %d is above %d" % (seq_len, MAX_SEQ_LEN))
    if token_type.shape[0] not in (1, 2):
        raise _lib.AnceLibraryError("token_type must have 1 or 2 rows, got %d" % token_type.shape[0])
    if padding_idx is not None and not 0 <= pad < vocab:
        raise _lib.AnceLibraryError("padding_idx must be in [0, %d), got %r" % (vocab, padding_idx))
    if position_mode == "roberta":
        if padding_idx is None:
            raise _lib.AnceLibraryError("position_mode \"roberta\" needs a padding_idx")
        if seq_len + pad + 1 > max_pos:
            raise _lib.AnceLibraryError("position table too small: L + padding_idx + 1 = %d > %d rows" % (seq_len + pad + 1, max_pos))
    elif seq_len > max_pos:
        raise _lib.AnceLibraryError("position table too small: L = %d > %d rows" % (seq_len, max_pos))
    if not 0.0 <= float(dropout_p) < 1.0:
        raise _lib.AnceLibraryError("dropout_p must be in [0, 1), got %r" % (dropout_p,))
    if not float(eps) > 0.0:
        raise _lib.AnceLibraryError("eps must be positive, got %r" % (eps,))
    return _BertEmbeddings.apply(word, position, token_type, ln_weight, ln_bias, input_ids, token_type_ids, float(eps),
                                 _lib.EMBED_POSITION_MODES[position_mode], pad, float(dropout_p), bool(training))


def bert_embeddings_packed(packed, word, position, token_type, ln_weight, ln_bias, eps, position_mode="absolute", padding_idx=None,
                           dropout_p=0.0, training=True):
    """``bert_embeddings`` over the R rows of a ``PackedTokens`` (``ance_amd.packing.pack_tokens`` with the same position_mode and
    padding_idx, which formed the positions) -> [R, H] fp32.  A row that a sequence covers has the bits of the padded call's row
    (dropout aside); a slack row is the embedding of a pad token: finite, and read by nothing that reaches a loss.  The dropout
    counter's row is the PACKED row index, so the masks are those of an R-row call.  The position table's gradient goes through the
    sorted positions in both modes; its padding row (roberta) and the word table's get no gradient, as in ``bert_embeddings``."""
    if not isinstance(packed, PackedTokens):
        raise _lib.AnceLibraryError("bert_embeddings_packed: packed must be a PackedTokens (ance_amd.packing.pack_tokens)")
    if not isinstance(word, torch.Tensor) or word.dim() != 2 or word.shape[1] not in TAIL_WIDTHS:
        raise _lib.AnceLibraryError("word must be [vocab, H] with H in %r" % (TAIL_WIDTHS,))
    H = word.shape[1]
    _check_table(word, "word", H)
    _check_table(position, "position", H, word)
    _check_table(token_type, "token_type", H, word)
    _check_vector(ln_weight, "ln_weight", H, word)
    _check_vector(ln_bias, "ln_bias", H, word)
    if packed.ids.device != word.device:
        raise _lib.AnceLibraryError("the packed batch must be on the word table's device")
    if position_mode not in _lib.EMBED_POSITION_MODES:
        raise _lib.AnceLibraryError("position_mode must be \"absolute\" or \"roberta\", got %r" % (position_mode,))
    vocab = word.shape[0]
    pad = -1 if padding_idx is None else int(padding_idx)
    if token_type.shape[0] not in (1, 2):
        raise _lib.AnceLibraryError("token_type must have 1 or 2 rows, got %d" % token_type.shape[0])
    if padding_idx is not None and not 0 <= pad < vocab:
        raise _lib.AnceLibraryError("padding_idx must be in [0, %d), got %r" % (vocab, padding_idx))
    if position_mode == "roberta" and padding_idx is None:
        raise _lib.AnceLibraryError("position_mode \"roberta\" needs a padding_idx")
    if not 0.0 <= float(dropout_p) < 1.0:
        raise _lib.AnceLibraryError("dropout_p must be in [0, 1), got %r" % (dropout_p,))
    if not float(eps) > 0.0:
        raise _lib.AnceLibraryError("eps must be positive, got %r" % (eps,))
    return _BertEmbeddingsRows.apply(word, position, token_type, ln_weight, ln_bias, packed.ids, packed.type_ids, packed.positions,
                                     float(eps), _lib.EMBED_POSITION_MODES[position_mode], pad, float(dropout_p), bool(training))


class BertEmbeddings(torch.nn.Module):
    """transformers' BertEmbeddings / RobertaEmbeddings with their parameter names -- word_embeddings.weight,
    position_embeddings.weight, token_type_embeddings.weight, LayerNorm.weight, LayerNorm.bias -- so that the ``embeddings.*`` part of
    a tower's state dict loads as it is (strict; the position_ids / token_type_ids buffers of recent transformers are not persistent
    and not in it).  ``forward(input_ids [B, L], token_type_ids=None) -> [B, L, H]`` is one bert_embeddings call.
    position_mode "roberta" needs pad_token_id; the parameters start as nn.Embedding / nn.LayerNorm initialise them."""

    def __init__(self, vocab_size, hidden_size, max_position_embeddings, type_vocab_size, layer_norm_eps=1e-12, hidden_dropout_prob=0.1,
                 pad_token_id=None, position_mode="absolute"):
        super().__init__()
        if hidden_size not in TAIL_WIDTHS or type_vocab_size not in (1, 2):
            raise _lib.AnceLibraryError("BertEmbeddings: hidden_size must be 768 or 1024 and type_vocab_size 1 or 2; got %r, %r"
                                        % (hidden_size, type_vocab_size))
        if position_mode not in _lib.EMBED_POSITION_MODES or (position_mode == "roberta" and pad_token_id is None):
            raise _lib.AnceLibraryError("BertEmbeddings: position_mode must be \"absolute\" or \"roberta\" (with a pad_token_id), got %r"
                                        % (position_mode,))
        nn = torch.nn
        self.position_mode, self.pad_token_id = position_mode, pad_token_id
        self.layer_norm_eps, self.hidden_dropout_prob = float(layer_norm_eps), float(hidden_dropout_prob)
        self.word_embeddings = nn.Embedding(vocab_size, hidden_size, padding_idx=pad_token_id)
        self.position_embeddings = nn.Embedding(max_position_embeddings, hidden_size,
                                                padding_idx=pad_token_id if position_mode == "roberta" else None)
        self.token_type_embeddings = nn.Embedding(type_vocab_size, hidden_size)
        self.LayerNorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)

    def forward(self, input_ids, token_type_ids=None):
        return bert_embeddings(input_ids, self.word_embeddings.weight, self.position_embeddings.weight,
                               self.token_type_embeddings.weight, self.LayerNorm.weight, self.LayerNorm.bias, self.layer_norm_eps,
                               token_type_ids, self.position_mode, self.pad_token_id, self.hidden_dropout_prob, self.training)

    def pack(self, input_ids, lens, rows, token_type_ids=None, dropped=None):
        """``pack_tokens`` with this module's position mode, padding index and table sizes."""
        from .packing import pack_tokens
        return pack_tokens(input_ids, lens, rows, token_type_ids, self.position_mode, self.pad_token_id,
                           self.word_embeddings.num_embeddings, self.position_embeddings.num_embeddings, dropped)

    @property
    def pack_rule(self):
        """The ``PackRule`` of ``pack``: what a PackedTokens for this module must have been made under."""
        return PackRule.of(self.position_mode, self.pad_token_id, self.word_embeddings.num_embeddings,
                           self.position_embeddings.num_embeddings)

    def forward_packed(self, packed):
        """[R, H] fp32 over the rows of a PackedTokens made under ``pack_rule`` (one bert_embeddings_packed call)."""
        return bert_embeddings_packed(packed, self.word_embeddings.weight, self.position_embeddings.weight,
                                      self.token_type_embeddings.weight, self.LayerNorm.weight, self.LayerNorm.bias, self.layer_norm_eps,
                                      self.position_mode, self.pad_token_id, self.hidden_dropout_prob, self.training)


class _Table(object):
    """What BertEmbeddings' methods read of a table that is not an nn.Embedding of its own."""
    __slots__ = ("weight",)

    def __init__(self, weight):
        self.weight = weight


class SeedEmbeddings(BertEmbeddings):
    """The input end of the SEED-Encoder's tower (fairseq's TransformerSentenceEncoder with num_segments = 0) under ITS parameter
    names -- embed_tokens.weight, embed_positions.weight, emb_layer_norm.weight / .bias -- so that ``named_parameters()`` and
    ``state_dict()`` are the reference's.  The arithmetic is BertEmbeddings' in roberta mode, unchanged: ``word_embeddings``,
    ``position_embeddings`` and ``LayerNorm`` are the three modules under their other names (properties, not registered twice), and
    the segment table is a non-persistent zero buffer [1, H] without a gradient -- ``(word + 0) + position`` is the same sum.
    There is no padded ``forward``: the tower masks keys by id, which only a batch packed by id (``pack``: ``pack_tokens_by_id``,
    rule "seed") expresses.  ``max_positions`` is the reference's: the position table has max_positions + padding_idx + 1 rows."""

    def __init__(self, vocab_size, hidden_size, max_positions, padding_idx=1, layer_norm_eps=1e-5, dropout=0.1):
        torch.nn.Module.__init__(self)
        if hidden_size not in TAIL_WIDTHS:
            raise _lib.AnceLibraryError("SeedEmbeddings: hidden_size must be 768 or 1024, got %r" % (hidden_size,))
        if padding_idx is None or not 0 <= int(padding_idx) < vocab_size:
            raise _lib.AnceLibraryError("SeedEmbeddings: padding_idx must be in [0, %d), got %r" % (vocab_size, padding_idx))
        nn = torch.nn
        self.position_mode, self.pad_token_id = "roberta", int(padding_idx)
        self.layer_norm_eps, self.hidden_dropout_prob = float(layer_norm_eps), float(dropout)
        self.embed_tokens = nn.Embedding(vocab_size, hidden_size, padding_idx=self.pad_token_id)
        self.embed_positions = nn.Embedding(max_positions + self.pad_token_id + 1, hidden_size, padding_idx=self.pad_token_id)
        self.emb_layer_norm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self.register_buffer("no_segment", torch.zeros(1, hidden_size), persistent=False)

    word_embeddings = property(lambda self: self.embed_tokens)
    position_embeddings = property(lambda self: self.embed_positions)
    LayerNorm = property(lambda self: self.emb_layer_norm)
    token_type_embeddings = property(lambda self: _Table(self.no_segment))

    def forward(self, input_ids, token_type_ids=None):
        raise _lib.AnceLibraryError("SeedEmbeddings has no padded form: pack by id (pack) and call forward_packed")

    def pack(self, input_ids, rows, dropped=None):
        """``pack_tokens_by_id`` with this module's padding index and table sizes."""
        from .packing import pack_tokens_by_id
        return pack_tokens_by_id(input_ids, rows, self.pad_token_id, self.embed_tokens.num_embeddings,
                                 self.embed_positions.num_embeddings, dropped)

    @property
    def pack_rule(self):
        return PackRule.of("seed", self.pad_token_id, self.embed_tokens.num_embeddings, self.embed_positions.num_embeddings)
