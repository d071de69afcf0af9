"""ctypes binding of the C-ABI in include/mbpe.h (libmbpe.so).

Used by tests/, bench.py and __graft_entry__.py.  The library itself is the
product; this file only marshals numpy arrays / device pointers into it.
There is no fallback: if libmbpe.so is missing, import-time use raises.
"""
import ctypes
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_PATH = os.environ.get("MBPE_LIB") or os.path.join(_PKG_DIR, "libmbpe.so")

OK = 0
NEED_EXCHANGE = 1
ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_VOCAB, ERR_STATE = -1, -2, -3, -4, -5
ERR_OOM, ERR_REGEX, ERR_SPLIT_GAP, ERR_COMM, ERR_OVERFLOW, ERR_IO = -6, -7, -8, -9, -10, -11
COMM_ID_BYTES = 128

# every symbol include/mbpe.h declares
EXPORTS = [
    "mbpe_last_error", "mbpe_version", "mbpe_create", "mbpe_destroy", "mbpe_load_corpus",
    "mbpe_pair_count_u8", "mbpe_train_begin", "mbpe_train_steps", "mbpe_train_sequences", "mbpe_train_result",
    "mbpe_train_lexical", "mbpe_train", "mbpe_get_stats", "mbpe_get_stream", "mbpe_stream_device", "mbpe_table_device", "mbpe_get_pairs", "mbpe_compact",
    "mbpe_set_option", "mbpe_comm_unique_id", "mbpe_comm_init", "mbpe_comm_init_external",
    "mbpe_comm_exchange_buffer", "mbpe_comm_exchange_done", "mbpe_presplit",
    "mbpe_split_count", "mbpe_split_offsets", "mbpe_split_has_gaps", "mbpe_split_starts", "mbpe_split_ends",
    "mbpe_split_free", "mbpe_load_corpus_ranges", "mbpe_split_pattern", "mbpe_encode_chunks",
    "mbpe_encode_chunks_device", "mbpe_decoder_create", "mbpe_decoder_destroy", "mbpe_decode_tokens",
    "mbpe_decode_slots", "mbpe_decoder_kernel_ms", "mbpe_decode_stream", "mbpe_encoder_create",
    "mbpe_encoder_destroy", "mbpe_encoder_encode", "mbpe_encoder_set_option", "mbpe_encoder_kernel_ms",
    "mbpe_encoder_alloc_count", "mbpe_encoder_pass_tokens", "mbpe_decode_batch", "mbpe_decoder_alloc_count",
    "mbpe_pack_tokens", "mbpe_unpack_tokens", "mbpe_pack_kernel_ms", "mbpe_encoder_encode_batch", "mbpe_encoder_pack_ms",
    "mbpe_pack_tokens_aux", "mbpe_pack_cu_seqlens", "mbpe_encoder_encode_batch_aux",
    "mbpe_load_corpus_endmask", "mbpe_splitter_create", "mbpe_splitter_destroy", "mbpe_splitter_split",
    "mbpe_splitter_endmask", "mbpe_splitter_set_option", "mbpe_splitter_kernel_ms", "mbpe_splitter_alloc_count",
    "mbpe_splitter_host_spans", "mbpe_splitter_split_docs", "mbpe_splitter_ranges", "mbpe_splitter_find_ms",
    "mbpe_encoder_encode_endmask", "mbpe_encoder_encode_batch_endmask", "mbpe_encoder_encode_byteoff",
    "mbpe_encoder_encode_endmask_byteoff", "mbpe_split_unicode_table",
    "mbpe_merges_check", "mbpe_train_begin_from", "mbpe_train_from",
    "mbpe_dropout_threshold", "mbpe_encoder_set_dropout",
    "mbpe_dedup_create", "mbpe_dedup_destroy", "mbpe_dedup_chunks_endmask", "mbpe_dedup_chunks", "mbpe_dedup_result",
    "mbpe_dedup_get", "mbpe_dedup_set_option", "mbpe_dedup_kernel_ms", "mbpe_dedup_alloc_count",
    "mbpe_load_corpus_weighted", "mbpe_load_corpus_endmask_weighted",
    "mbpe_dedup_map", "mbpe_dedup_get_map", "mbpe_encoder_dedup_stats",
    "mbpe_wordcount_create", "mbpe_wordcount_destroy", "mbpe_wordcount_add_endmask", "mbpe_wordcount_add",
    "mbpe_wordcount_result", "mbpe_wordcount_get", "mbpe_wordcount_stats", "mbpe_wordcount_reset",
    "mbpe_wordcount_set_option", "mbpe_wordcount_kernel_ms", "mbpe_wordcount_alloc_count",
    "mbpe_wordcount_export_size", "mbpe_wordcount_export", "mbpe_wordcount_merge_blob", "mbpe_wordcount_merge",
    "mbpe_pack_windows", "mbpe_encoder_encode_batch_windows", "mbpe_encoder_encode_batch_endmask_windows",
    "mbpe_token_counts", "mbpe_token_counts_kernel_ms", "mbpe_encoder_count", "mbpe_encoder_count_endmask",
    "mbpe_encoder_counts", "mbpe_encoder_counts_reset",
    "mbpe_pack_fit", "mbpe_pack_fit_plan", "mbpe_pack_fit_cu_seqlens", "mbpe_encoder_encode_batch_fit",
    "mbpe_encoder_encode_batch_endmask_fit",
    "mbpe_fim_plan", "mbpe_fim_tokens", "mbpe_fim_kernel_ms", "mbpe_encoder_set_fim", "mbpe_encoder_fim_info",
    "mbpe_mlm_plan", "mbpe_mlm_tokens", "mbpe_mlm_kernel_ms", "mbpe_pack_tokens_aux_labels", "mbpe_pack_windows_labels",
    "mbpe_pack_fit_labels", "mbpe_encoder_set_mlm",
    "mbpe_denoise_plan", "mbpe_denoise_tokens", "mbpe_denoise_kernel_ms", "mbpe_encoder_encode_batch_denoise",
    "mbpe_encoder_encode_batch_endmask_denoise",
]
# include/mbpe_tokenizer.h
TOK_EXPORTS = [
    "mbpe_tok_create", "mbpe_tok_destroy", "mbpe_tok_set_special_tokens", "mbpe_tok_train", "mbpe_tok_set_merges",
    "mbpe_tok_get_merges", "mbpe_tok_save", "mbpe_tok_load", "mbpe_tok_encode", "mbpe_tok_encode_device",
    "mbpe_tok_decode", "mbpe_tok_decode_device", "mbpe_tok_encode_batch_device", "mbpe_tok_decode_batch_device",
    "mbpe_tok_encode_batch_packed_device", "mbpe_tok_decode_padded_device", "mbpe_tok_encode_batch_aux_device",
    "mbpe_tok_train_split_device", "mbpe_tok_set_encode_split", "mbpe_tok_set_split_unicode",
    "mbpe_tok_set_encode_order", "mbpe_tok_train_continue", "mbpe_tok_encode_byteoff",
    "mbpe_tok_encode_batch_byteoff_device", "mbpe_tok_set_encode_dropout", "mbpe_tok_set_train_dedup",
    "mbpe_tok_set_encode_dedup", "mbpe_tok_train_pieces_begin", "mbpe_tok_train_pieces_add",
    "mbpe_tok_train_pieces_finish", "mbpe_tok_train_pieces_abort", "mbpe_tok_set_train_limits",
    "mbpe_tok_train_pieces_export_size", "mbpe_tok_train_pieces_export", "mbpe_tok_train_pieces_merge",
    "mbpe_tok_encode_batch_windows_device", "mbpe_tok_count_tokens", "mbpe_tok_token_counts",
    "mbpe_tok_token_counts_reset", "mbpe_tok_encode_batch_fit_device", "mbpe_tok_set_encode_fim",
    "mbpe_tok_encode_fim_info", "mbpe_tok_set_encode_mlm", "mbpe_tok_encode_batch_denoise_device",
]


class Stats(ctypes.Structure):
    _fields_ = [
        ("n_bytes", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64), ("n_slots", ctypes.c_uint64),
        ("n_live", ctypes.c_uint64), ("n_merges", ctypes.c_uint32), ("n_compactions", ctypes.c_uint32),
        ("n_pairs", ctypes.c_uint64), ("ms_pair_count", ctypes.c_float), ("ms_begin", ctypes.c_float),
        ("ms_steps", ctypes.c_float), ("pair_count_launches", ctypes.c_uint32), ("merge_launches", ctypes.c_uint32),
        ("ms_merge_kernel", ctypes.c_float), ("n_batches", ctypes.c_uint32),
        ("n_fused", ctypes.c_uint32), ("n_fused_dropped", ctypes.c_uint32), ("cut_conflict", ctypes.c_uint32),
        ("cut_bucket", ctypes.c_uint32), ("cut_single", ctypes.c_uint32), ("cut_full", ctypes.c_uint32),
        ("n_validation_drops", ctypes.c_uint32), ("ms_grow_table", ctypes.c_float), ("ms_compact", ctypes.c_float),
        ("n_table_grows", ctypes.c_uint32), ("n_sel_fallback", ctypes.c_uint32),
        ("fused_launches", ctypes.c_uint32), ("ms_fused_kernel", ctypes.c_float), ("fused_slots", ctypes.c_uint64),
        ("n_sel_retry", ctypes.c_uint32), ("adapt_limit", ctypes.c_uint32), ("n_sel_blocks", ctypes.c_uint64), ("size_hist", ctypes.c_uint32 * 8),
        ("n_skipped", ctypes.c_uint32), ("n_skip_cut", ctypes.c_uint32),
        ("exchange_words", ctypes.c_uint64), ("exchanges", ctypes.c_uint32), ("log_spilled", ctypes.c_uint32),
        ("fused_live_tokens", ctypes.c_uint64), ("ms_pair_count_kernel", ctypes.c_float), ("log_passes", ctypes.c_uint32),
        ("log_refills", ctypes.c_uint32), ("pad3_", ctypes.c_uint32),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["size_hist"] = list(self.size_hist)
        return d



PACK_PADDED, PACK_PACKED = 0, 1
SPLIT_BLOCK, SPLIT_TILE, SPLIT_MAX_SPAN = 64, 16384, 4096      # MBPE_SPLIT_BLOCK, _TILE, _MAX_SPAN
NO_TOKEN = 0xFFFFFFFF


class PackSpec(ctypes.Structure):
    """mbpe_pack_spec (include/mbpe.h)."""
    _fields_ = [
        ("layout", ctypes.c_uint32), ("seq_len", ctypes.c_uint32), ("out_bits", ctypes.c_uint32),
        ("pad_id", ctypes.c_uint32), ("bos_id", ctypes.c_uint32), ("eos_id", ctypes.c_uint32),
        ("pad_left", ctypes.c_uint32), ("trunc_left", ctypes.c_uint32),
    ]


class PackAux(ctypes.Structure):
    """mbpe_pack_aux (include/mbpe.h): where labels, positions and segments go (NULL: not asked for)."""
    _fields_ = [
        ("labels", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("seg", ctypes.c_void_p),
        ("ignore_label", ctypes.c_int64),
    ]


class PackWindow(ctypes.Structure):
    """mbpe_pack_window (include/mbpe.h): how the windows of a long document overlap, and where the rows' document
    numbers and first-token indices go (NULL: not asked for)."""
    _fields_ = [
        ("stride", ctypes.c_uint32), ("score_once", ctypes.c_uint32), ("row_doc", ctypes.c_void_p),
        ("row_tok0", ctypes.c_void_p),
    ]


class PackFit(ctypes.Structure):
    """struct mbpe_pack_fit (include/mbpe.h): where the cell of every document's last piece goes (NULL: not asked
    for)."""
    _fields_ = [("doc_row", ctypes.c_void_p), ("doc_col", ctypes.c_void_p)]


class FimSpec(ctypes.Structure):
    """mbpe_fim_spec (include/mbpe.h): the fill-in-the-middle transform; fim_spec() makes one from rates."""
    _fields_ = [
        ("rate", ctypes.c_uint64), ("spm", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("doc_base", ctypes.c_uint64),
        ("pre_id", ctypes.c_uint32), ("suf_id", ctypes.c_uint32), ("mid_id", ctypes.c_uint32),
        ("min_tokens", ctypes.c_uint32), ("max_tokens", ctypes.c_uint32),
    ]


FIM_NONE, FIM_PSM, FIM_SPM = 0, 1, 2      # the modes of fim_plan / fim_info


class MlmSpec(ctypes.Structure):
    """mbpe_mlm_spec (include/mbpe.h): masked-LM corruption; mlm_spec() makes one from rates."""
    _fields_ = [
        ("select", ctypes.c_uint64), ("mask", ctypes.c_uint64), ("random", ctypes.c_uint64), ("seed", ctypes.c_uint64),
        ("doc_base", ctypes.c_uint64), ("mask_id", ctypes.c_uint32), ("vocab_n", ctypes.c_uint32),
        ("whole_word", ctypes.c_uint32), ("n_protect", ctypes.c_uint32), ("protect", ctypes.c_uint32 * 8),
    ]


class DenoiseSpec(ctypes.Structure):
    """mbpe_denoise_spec (include/mbpe.h): span corruption for encoder-decoder models; denoise_spec() makes one."""
    _fields_ = [
        ("density", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("doc_base", ctypes.c_uint64),
        ("mean_span_q8", ctypes.c_uint32), ("segment_tokens", ctypes.c_uint32), ("min_tokens", ctypes.c_uint32),
        ("sentinel_id", ctypes.c_uint32), ("sentinel_down", ctypes.c_uint32), ("n_sentinels", ctypes.c_uint32),
    ]


class DenoiseBatch(ctypes.Structure):
    """mbpe_denoise_batch (include/mbpe.h): where the two matrices of a denoise batch call go (NULL: not asked for)."""
    _fields_ = [
        ("enc_ids", ctypes.c_void_p), ("enc_len", ctypes.c_void_p), ("dec_ids", ctypes.c_void_p),
        ("dec_len", ctypes.c_void_p), ("dec_labels", ctypes.c_void_p), ("row_doc", ctypes.c_void_p),
        ("ignore_label", ctypes.c_int64),
    ]


_ID_DTYPES = {16: np.uint16, 32: np.uint32, 64: np.uint64}
# labels are ids or ignore_label: signed where a negative ignore_label fits
_LABEL_DTYPES = {16: np.uint16, 32: np.int32, 64: np.int64}


def pack_spec(seq_len, layout="padded", out_bits=32, pad_id=0, bos_id=None, eos_id=None, pad_left=False,
              trunc_left=False):
    """A PackSpec from keywords; layout "padded" / "packed" (or the number), bos_id / eos_id None = none."""
    if isinstance(layout, str):
        if layout not in ("padded", "packed"):
            raise ValueError("layout must be \"padded\" or \"packed\"")
        layout = PACK_PADDED if layout == "padded" else PACK_PACKED
    return PackSpec(layout, seq_len, out_bits, pad_id, NO_TOKEN if bos_id is None else bos_id,
                    NO_TOKEN if eos_id is None else eos_id, int(bool(pad_left)), int(bool(trunc_left)))


class MbpeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mbpe error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmbpe.so is not built (%s); run __graft_entry__.build()" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, u32, i32, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int64
    L.mbpe_last_error.restype = ctypes.c_char_p
    L.mbpe_version.restype = ctypes.c_char_p
    L.mbpe_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.mbpe_destroy.argtypes = [vp]
    L.mbpe_destroy.restype = None
    L.mbpe_load_corpus.argtypes = [vp, vp, u64, vp, u64, i32]
    L.mbpe_pair_count_u8.argtypes = [vp, vp]
    L.mbpe_train_begin.argtypes = [vp, u32]
    L.mbpe_train_steps.argtypes = [vp, u32, vp]
    L.mbpe_train_sequences.argtypes = [vp, u32, vp]
    L.mbpe_train_result.argtypes = [vp, vp, vp, u32, vp]
    L.mbpe_train_lexical.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp, vp, vp]
    L.mbpe_train.argtypes = [vp, vp, u64, vp, u64, u32, i32, vp, vp, vp, vp]
    L.mbpe_merges_check.argtypes = [vp, u32]
    L.mbpe_train_begin_from.argtypes = [vp, u32, vp, u32]
    L.mbpe_train_from.argtypes = [vp, vp, u64, vp, u64, u32, i32, vp, u32, vp, vp, vp, vp]
    L.mbpe_get_stats.argtypes = [vp, vp]
    L.mbpe_get_stream.argtypes = [vp, vp, vp, u64, vp]
    L.mbpe_stream_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(u32), ctypes.POINTER(u32),
                                     ctypes.POINTER(u32)]
    L.mbpe_table_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u32)]
    L.mbpe_get_pairs.argtypes = [vp, vp, vp, vp, u64, vp]
    L.mbpe_compact.argtypes = [vp]
    L.mbpe_set_option.argtypes = [vp, ctypes.c_char_p, i64]
    L.mbpe_comm_unique_id.argtypes = [vp]
    L.mbpe_comm_init.argtypes = [vp, vp, i32, i32]
    L.mbpe_comm_init_external.argtypes = [vp, i32, i32]
    L.mbpe_comm_exchange_buffer.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64)]
    L.mbpe_comm_exchange_done.argtypes = [vp]
    L.mbpe_presplit.argtypes = [ctypes.c_char_p, vp, u64, ctypes.POINTER(vp)]
    L.mbpe_split_count.argtypes = [vp]
    L.mbpe_split_count.restype = u64
    L.mbpe_split_offsets.argtypes = [vp]
    L.mbpe_split_offsets.restype = ctypes.POINTER(ctypes.c_uint64)
    L.mbpe_split_has_gaps.argtypes = [vp]
    L.mbpe_split_starts.argtypes = [vp]
    L.mbpe_split_starts.restype = ctypes.POINTER(ctypes.c_uint64)
    L.mbpe_split_ends.argtypes = [vp]
    L.mbpe_split_ends.restype = ctypes.POINTER(ctypes.c_uint64)
    L.mbpe_load_corpus_ranges.argtypes = [vp, vp, u64, vp, vp, u64, i32]
    L.mbpe_split_free.argtypes = [vp]
    L.mbpe_split_free.restype = None
    L.mbpe_split_pattern.argtypes = [ctypes.c_char_p]
    L.mbpe_split_pattern.restype = ctypes.c_char_p
    L.mbpe_encode_chunks.argtypes = [i32, vp, u64, vp, u64, vp, u32, vp, u64, vp, vp]
    L.mbpe_encode_chunks_device.argtypes = [i32, vp, u64, vp, u64, vp, u32, vp, u64, vp, vp]
    L.mbpe_encoder_create.argtypes = [i32, vp, u32, ctypes.POINTER(vp)]
    L.mbpe_encoder_destroy.argtypes = [vp]
    L.mbpe_encoder_destroy.restype = None
    L.mbpe_encoder_encode.argtypes = [vp, vp, u64, i32, vp, u64, vp, u64, u32, i32, vp, vp, vp]
    L.mbpe_encoder_set_option.argtypes = [vp, ctypes.c_char_p, i64]
    L.mbpe_encoder_kernel_ms.argtypes = [vp, vp]
    L.mbpe_encoder_alloc_count.argtypes = [vp, vp]
    L.mbpe_encoder_pass_tokens.argtypes = [vp, vp, u32, vp]
    L.mbpe_pack_tokens.argtypes = [i32, vp, u64, u32, i32, vp, u64, vp, vp, u64, i32, vp, vp]
    L.mbpe_unpack_tokens.argtypes = [i32, vp, u64, u32, u32, i32, vp, vp, u64, u32, i32, vp, vp]
    L.mbpe_pack_kernel_ms.argtypes = [vp]
    L.mbpe_encoder_encode_batch.argtypes = [vp, vp, u64, i32, vp, u64, vp, u64, vp, vp, u64, i32, vp, vp, vp]
    L.mbpe_encoder_pack_ms.argtypes = [vp, vp]
    L.mbpe_pack_tokens_aux.argtypes = L.mbpe_pack_tokens.argtypes + [vp]
    L.mbpe_pack_cu_seqlens.argtypes = [vp, u64, vp, vp, u64, vp, vp]
    L.mbpe_encoder_encode_batch_aux.argtypes = L.mbpe_encoder_encode_batch.argtypes + [vp, vp]
    L.mbpe_tok_encode_batch_packed_device.argtypes = [vp, vp, vp, u64, i32, i32, vp, vp, u64, i32, vp, vp, vp]
    L.mbpe_tok_encode_batch_aux_device.argtypes = L.mbpe_tok_encode_batch_packed_device.argtypes + [vp, vp]
    L.mbpe_pack_windows.argtypes = L.mbpe_pack_tokens_aux.argtypes + [vp]
    L.mbpe_encoder_encode_batch_windows.argtypes = L.mbpe_encoder_encode_batch_aux.argtypes + [vp]
    L.mbpe_tok_encode_batch_windows_device.argtypes = L.mbpe_tok_encode_batch_aux_device.argtypes + [vp]
    L.mbpe_pack_fit.argtypes = L.mbpe_pack_tokens_aux.argtypes + [vp]
    L.mbpe_pack_fit_plan.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp]
    L.mbpe_pack_fit_cu_seqlens.argtypes = L.mbpe_pack_cu_seqlens.argtypes
    L.mbpe_encoder_encode_batch_fit.argtypes = L.mbpe_encoder_encode_batch_aux.argtypes + [vp]
    L.mbpe_tok_encode_batch_fit_device.argtypes = L.mbpe_tok_encode_batch_aux_device.argtypes + [vp]
    L.mbpe_tok_decode_padded_device.argtypes = [vp, vp, u64, u32, vp, i32, i32, vp, u64, vp, vp]
    L.mbpe_tok_encode_batch_device.argtypes = [vp, vp, vp, u64, i32, i32, vp, u64, vp, vp]
    L.mbpe_decoder_create.argtypes = [i32, vp, u32, vp, vp, vp, u32, ctypes.POINTER(vp)]
    L.mbpe_decoder_destroy.argtypes = [vp]
    L.mbpe_decoder_destroy.restype = None
    L.mbpe_decode_tokens.argtypes = [vp, vp, u64, i32, vp, u64, i32, vp, vp]
    L.mbpe_decode_slots.argtypes = [vp, vp, u64, u32, u32, u32, vp, u64, i32, vp, vp]
    L.mbpe_decoder_kernel_ms.argtypes = [vp, vp]
    L.mbpe_decode_batch.argtypes = [vp, vp, u64, u32, i32, vp, u64, vp, u64, i32, vp, vp, vp]
    L.mbpe_decoder_alloc_count.argtypes = [vp, vp]
    L.mbpe_tok_decode_batch_device.argtypes = [vp, vp, vp, u64, i32, i32, vp, u64, vp, vp]
    L.mbpe_decode_stream.argtypes = [vp, vp, u64, i32, vp]
    L.mbpe_tok_decode_device.argtypes = [vp, vp, u64, i32, i32, vp, u64, vp]
    L.mbpe_tok_create.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.mbpe_tok_destroy.argtypes = [vp]
    L.mbpe_tok_destroy.restype = None
    L.mbpe_tok_set_special_tokens.argtypes = [vp, ctypes.c_char_p, u64]
    L.mbpe_tok_train.argtypes = [vp, vp, u64, u32, i32, i32, i32]
    L.mbpe_tok_train_split_device.argtypes = L.mbpe_tok_train.argtypes
    L.mbpe_tok_train_continue.argtypes = L.mbpe_tok_train.argtypes + [i32]
    L.mbpe_load_corpus_endmask.argtypes = [vp, vp, u64, i32, vp]
    L.mbpe_splitter_create.argtypes = [i32, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.mbpe_splitter_destroy.argtypes = [vp]
    L.mbpe_splitter_destroy.restype = None
    L.mbpe_splitter_split.argtypes = [vp, vp, u64, i32, vp, vp, u64, vp]
    L.mbpe_splitter_endmask.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(vp)]
    L.mbpe_splitter_set_option.argtypes = [vp, ctypes.c_char_p, i64]
    L.mbpe_splitter_kernel_ms.argtypes = [vp, vp]
    L.mbpe_splitter_alloc_count.argtypes = [vp, vp]
    L.mbpe_splitter_host_spans.argtypes = [vp, vp, vp]
    L.mbpe_splitter_split_docs.argtypes = [vp, vp, u64, i32, vp, u64, vp, vp, u32, vp, vp, u64, vp, vp]
    L.mbpe_splitter_ranges.argtypes = [vp, vp, vp]
    L.mbpe_splitter_find_ms.argtypes = [vp, vp]
    L.mbpe_encoder_encode_endmask.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, u32, i32, vp, vp, vp]
    L.mbpe_encoder_encode_endmask_byteoff.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, u64, u32, i32, vp, vp, vp, vp]
    L.mbpe_encoder_encode_byteoff.argtypes = [vp, vp, u64, i32, vp, u64, vp, u64, u32, i32, vp, vp, vp, vp]
    L.mbpe_tok_encode_byteoff.argtypes = [vp, vp, u64, i32, i32, vp, vp, u64, vp]
    L.mbpe_tok_encode_batch_byteoff_device.argtypes = [vp, vp, vp, u64, i32, i32, vp, vp, u64, vp, vp]
    L.mbpe_encoder_encode_batch_endmask.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, u64, i32, vp, vp, vp,
                                                    vp, vp]
    L.mbpe_encoder_encode_batch_endmask_windows.argtypes = L.mbpe_encoder_encode_batch_endmask.argtypes + [vp]
    L.mbpe_encoder_encode_batch_endmask_fit.argtypes = L.mbpe_encoder_encode_batch_endmask.argtypes + [vp]
    L.mbpe_tok_set_encode_split.argtypes = [vp, i32]
    L.mbpe_tok_set_split_unicode.argtypes = [vp, i32]
    L.mbpe_tok_set_train_dedup.argtypes = [vp, i32]
    L.mbpe_tok_set_train_limits.argtypes = [vp, ctypes.c_int64, ctypes.c_int64]
    L.mbpe_dedup_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.mbpe_dedup_destroy.argtypes = [vp]
    L.mbpe_dedup_destroy.restype = None
    L.mbpe_dedup_chunks_endmask.argtypes = [vp, vp, u64, vp, vp, vp]
    L.mbpe_dedup_chunks.argtypes = [vp, vp, u64, i32, vp, u64, vp, vp]
    L.mbpe_dedup_result.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mbpe_dedup_get.argtypes = [vp, vp, vp, vp, vp, u64, u64]
    L.mbpe_dedup_set_option.argtypes = [vp, ctypes.c_char_p, i64]
    L.mbpe_dedup_kernel_ms.argtypes = [vp, vp]
    L.mbpe_dedup_alloc_count.argtypes = [vp, vp]
    L.mbpe_dedup_map.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64)]
    L.mbpe_dedup_get_map.argtypes = [vp, vp, u64, vp]
    L.mbpe_encoder_dedup_stats.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mbpe_tok_set_encode_dedup.argtypes = [vp, i32]
    L.mbpe_wordcount_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.mbpe_wordcount_destroy.argtypes = [vp]
    L.mbpe_wordcount_destroy.restype = None
    L.mbpe_wordcount_add_endmask.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.mbpe_wordcount_add.argtypes = [vp, vp, u64, i32, vp, u64, u32, vp, vp]
    L.mbpe_wordcount_result.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mbpe_wordcount_get.argtypes = [vp, vp, vp, vp, vp, u64, u64]
    L.mbpe_wordcount_stats.argtypes = [vp, vp, vp, vp, vp]
    L.mbpe_wordcount_reset.argtypes = [vp]
    L.mbpe_wordcount_set_option.argtypes = [vp, ctypes.c_char_p, i64]
    L.mbpe_wordcount_kernel_ms.argtypes = [vp, vp]
    L.mbpe_wordcount_alloc_count.argtypes = [vp, vp]
    L.mbpe_wordcount_export_size.argtypes = [vp, vp]
    L.mbpe_wordcount_export.argtypes = [vp, vp, u64, vp]
    L.mbpe_wordcount_merge_blob.argtypes = [vp, vp, u64, vp, vp]
    L.mbpe_wordcount_merge.argtypes = [vp, vp]
    L.mbpe_tok_train_pieces_export_size.argtypes = [vp, vp]
    L.mbpe_tok_train_pieces_export.argtypes = [vp, vp, u64, vp]
    L.mbpe_tok_train_pieces_merge.argtypes = [vp, vp, u64]
    L.mbpe_tok_train_pieces_begin.argtypes = [vp, i32, i32]
    L.mbpe_tok_train_pieces_add.argtypes = [vp, vp, u64, u32]
    L.mbpe_tok_train_pieces_finish.argtypes = [vp, u32, i32, i32, i32]
    L.mbpe_tok_train_pieces_abort.argtypes = [vp]
    L.mbpe_load_corpus_weighted.argtypes = [vp, vp, u64, vp, u64, i32, vp]
    L.mbpe_load_corpus_endmask_weighted.argtypes = [vp, vp, u64, i32, vp, vp, u64, i32]
    L.mbpe_tok_set_encode_order.argtypes = [vp, i32]
    L.mbpe_dropout_threshold.argtypes = [ctypes.c_double, vp]
    L.mbpe_encoder_set_dropout.argtypes = [vp, u64, u64]
    L.mbpe_tok_set_encode_dropout.argtypes = [vp, u64, u64]
    L.mbpe_split_unicode_table.argtypes = [vp, vp, vp, u32, vp, vp]
    L.mbpe_tok_set_merges.argtypes = [vp, vp, u32]
    L.mbpe_tok_get_merges.argtypes = [vp, vp, u32, vp]
    L.mbpe_tok_save.argtypes = [vp, ctypes.c_char_p, i32]
    L.mbpe_tok_load.argtypes = [vp, ctypes.c_char_p, i32]
    L.mbpe_tok_encode.argtypes = [vp, vp, u64, i32, vp, u64, vp]
    L.mbpe_tok_encode_device.argtypes = [vp, vp, u64, i32, i32, vp, u64, vp]
    L.mbpe_tok_decode.argtypes = [vp, vp, u64, i32, vp, u64, vp]
    L.mbpe_token_counts.argtypes = [i32, vp, u64, u32, i32, vp, u64, i32, vp]
    L.mbpe_token_counts_kernel_ms.argtypes = [vp]
    L.mbpe_encoder_count.argtypes = [vp, vp, u64, i32, vp, u64, u64, vp, vp]
    L.mbpe_encoder_count_endmask.argtypes = [vp, vp, u64, vp, vp, u64, u64, vp, vp]
    L.mbpe_encoder_counts.argtypes = [vp, vp, u64, i32, vp, vp, vp]
    L.mbpe_encoder_counts_reset.argtypes = [vp]
    L.mbpe_tok_count_tokens.argtypes = [vp, vp, vp, u64, i32, i32, u64, vp]
    L.mbpe_tok_token_counts.argtypes = [vp, vp, u64, vp, vp]
    L.mbpe_tok_token_counts_reset.argtypes = [vp]
    L.mbpe_denoise_plan.argtypes = [vp, u64, vp, vp, vp, vp, vp, u64]
    L.mbpe_denoise_tokens.argtypes = [i32, vp, u64, u32, i32, vp, u64, vp, vp, u64, vp, u64, i32, vp, vp, vp, u64, vp, vp,
                                      vp]
    L.mbpe_denoise_kernel_ms.argtypes = [vp]
    L.mbpe_encoder_encode_batch_denoise.argtypes = [vp, vp, u64, i32, vp, u64, vp, u64, vp, vp, vp, vp, u64, i32, vp, vp]
    L.mbpe_encoder_encode_batch_endmask_denoise.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp, vp, u64, i32,
                                                            vp, vp]
    L.mbpe_tok_encode_batch_denoise_device.argtypes = [vp, vp, vp, u64, i32, i32, vp, vp, vp, vp, u64, i32, vp, vp]
    L.mbpe_fim_plan.argtypes = [vp, u64, vp, vp, vp, vp]
    L.mbpe_fim_tokens.argtypes = [i32, vp, u64, u32, i32, vp, u64, vp, vp, u64, i32, vp, vp]
    L.mbpe_fim_kernel_ms.argtypes = [vp]
    L.mbpe_encoder_set_fim.argtypes = [vp, vp]
    L.mbpe_encoder_fim_info.argtypes = [vp, vp, vp, u64, vp]
    L.mbpe_tok_set_encode_fim.argtypes = [vp, vp]
    L.mbpe_tok_encode_fim_info.argtypes = [vp, vp, vp, u64, vp]
    L.mbpe_mlm_plan.argtypes = [vp, u64, u32, vp, u64, vp, vp, vp]
    L.mbpe_mlm_tokens.argtypes = [i32, vp, u64, u32, i32, vp, u64, vp, vp, vp, i32]
    L.mbpe_mlm_kernel_ms.argtypes = [vp]
    L.mbpe_pack_tokens_aux_labels.argtypes = L.mbpe_pack_tokens_aux.argtypes + [vp]
    L.mbpe_pack_windows_labels.argtypes = L.mbpe_pack_windows.argtypes + [vp]
    L.mbpe_pack_fit_labels.argtypes = L.mbpe_pack_fit.argtypes + [vp]
    L.mbpe_encoder_set_mlm.argtypes = [vp, vp]
    L.mbpe_tok_set_encode_mlm.argtypes = [vp, vp]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise MbpeError(rc, lib().mbpe_last_error().decode("utf-8", "replace"))
    return rc


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(data, dtype=np.uint8)


def _merges(merges):
    return np.ascontiguousarray([] if merges is None else merges, dtype=np.uint32).reshape(-1, 2)


def merges_check(merges):
    """mbpe_merges_check: raises MbpeError(ERR_ARG), naming the first offending index, unless both sides of merge k are
    below 256 + k and no pair occurs twice (a trained table).  Host only."""
    m = _merges(merges)
    _check(lib().mbpe_merges_check(m.ctypes.data if len(m) else None, len(m)))


def split_pattern(encoder):
    p = lib().mbpe_split_pattern(encoder.encode())
    if p is None:
        raise ValueError("Encoder should be one of: basic, gpt2 or gpt4")
    return p.decode("utf-8")


def split_unicode_table():
    """What PCRE2 says of every code point (mbpe_split_unicode_table) -> (classes as uint32[0x110000 / 16], 2 bits per
    code point: 0 L, 1 N, 2 S, 3 other; {code point >= 0x80: the letter of "sdmtlver" it folds to}; build time in ms)."""
    cls = np.zeros(0x110000 // 16, dtype=np.uint32)
    cp, to = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    n, ms = ctypes.c_uint32(), ctypes.c_double()
    _check(lib().mbpe_split_unicode_table(cls.ctypes.data, cp.ctypes.data, to.ctypes.data, 8, ctypes.byref(n),
                                          ctypes.byref(ms)))
    return cls, {int(cp[k]): chr(to[k]) for k in range(n.value)}, ms.value


def presplit_ranges(pattern, data):
    """The same as (starts, ends) arrays: chunks need not tile the text (bytes between matches are skipped)."""
    text = _u8(data)
    h = ctypes.c_void_p()
    _check(lib().mbpe_presplit(pattern.encode("utf-8"), text.ctypes.data if len(text) else None,
                               len(text), ctypes.byref(h)))
    try:
        n = lib().mbpe_split_count(h)
        if n == 0:
            return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
        return (np.ctypeslib.as_array(lib().mbpe_split_starts(h), shape=(n,)).copy(),
                np.ctypeslib.as_array(lib().mbpe_split_ends(h), shape=(n,)).copy())
    finally:
        lib().mbpe_split_free(h)


def presplit(pattern, data):
    """Tokenizer::train's regex pre-split (Tokenizer.h:500-540) -> uint64 offsets [n_chunks+1]."""
    text = _u8(data)
    h = ctypes.c_void_p()
    _check(lib().mbpe_presplit(pattern.encode("utf-8"), text.ctypes.data if len(text) else None,
                               len(text), ctypes.byref(h)))
    try:
        n = lib().mbpe_split_count(h)
        p = lib().mbpe_split_offsets(h)
        if not p:
            raise MbpeError(ERR_SPLIT_GAP, lib().mbpe_last_error().decode("utf-8", "replace"))
        return np.ctypeslib.as_array(p, shape=(n + 1,)).copy()
    finally:
        lib().mbpe_split_free(h)


def encode_chunks(data, chunk_off, merges, device=0):
    """internal_encode on the device (mbpe_encode_chunks) -> (uint32 tokens, passes)."""
    text = _u8(data)
    off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
    m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
    n, passes = ctypes.c_uint64(), ctypes.c_uint32()
    out = np.zeros(max(len(text), 1), dtype=np.uint32)
    _check(lib().mbpe_encode_chunks(device, text.ctypes.data if len(text) else None, len(text),
                                    None if off is None else off.ctypes.data, 0 if off is None else len(off) - 1,
                                    m.ctypes.data if len(m) else None, len(m), out.ctypes.data, len(out),
                                    ctypes.byref(n), ctypes.byref(passes)))
    return out[:n.value].copy(), passes.value


def encode_chunks_device(data, chunk_off, merges, out_ptr, cap, device=0):
    """mbpe_encode_chunks_device: the tokens (bit 31 = chunk end) go to device memory at out_ptr (room for cap
    tokens; 0 to query) -> (token count, passes)."""
    text = _u8(data)
    off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
    m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
    n, passes = ctypes.c_uint64(), ctypes.c_uint32()
    _check(lib().mbpe_encode_chunks_device(device, text.ctypes.data if len(text) else None, len(text),
                                           None if off is None else off.ctypes.data, 0 if off is None else len(off) - 1,
                                           m.ctypes.data if len(m) else None, len(m),
                                           ctypes.c_void_p(out_ptr) if out_ptr else None, cap,
                                           ctypes.byref(n), ctypes.byref(passes)))
    return n.value, passes.value


def _ptr(p):
    return ctypes.c_void_p(p) if p else None


def _matrix(n_rows, spec):
    """Host arrays for n_rows rows of a spec: (ids [n_rows, seq_len], lengths [n_rows])."""
    return (np.zeros((n_rows, spec.seq_len), dtype=_ID_DTYPES[spec.out_bits]), np.zeros(n_rows, dtype=np.uint32))


def pack_tokens(tokens, doc_tok_off, seq_len, layout="padded", out_bits=32, pad_id=0, bos_id=None, eos_id=None,
                pad_left=False, trunc_left=False, device=0, tokens_ptr=None, n_tokens=None, token_bits=None,
                out_ptr=None, len_ptr=None, cap_rows=None):
    """mbpe_pack_tokens: a flat token array (uint16 or uint32) whose document i is tokens[doc_tok_off[i]:
    doc_tok_off[i + 1]] -> (ids [n_rows, seq_len] of out_bits bits, lengths [n_rows]) as numpy arrays.
    Device memory: tokens_ptr= / n_tokens= / token_bits= name the tokens there instead of `tokens`; with out_ptr= (and
    len_ptr=, room for cap_rows rows) the matrix is written there and the row count is returned."""
    spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    if tokens_ptr is None:
        t = np.ascontiguousarray(tokens)
        if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            t = t.astype(np.uint32)
        t = t.reshape(-1)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    n_rows = ctypes.c_uint64()
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    if out_ptr is not None:
        _check(lib().mbpe_pack_tokens(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), ctypes.byref(n_rows)))
        return n_rows.value
    _check(lib().mbpe_pack_tokens(*head, None, 0, 0, None, ctypes.byref(n_rows)))
    ids, lengths = _matrix(n_rows.value, spec)
    if n_rows.value:
        _check(lib().mbpe_pack_tokens(*head, ids.ctypes.data, n_rows.value, 0, lengths.ctypes.data,
                                      ctypes.byref(n_rows)))
    return ids, lengths


def fim_spec(rate, spm_rate, pre_id, suf_id, mid_id, seed=0, doc_base=0, min_tokens=0, max_tokens=0):
    """A FimSpec from probabilities: a document is transformed with probability `rate`, a transformed one is SPM with
    probability spm_rate (else PSM); pre_id / suf_id / mid_id are the sentinel ids; seed picks the epoch's draw,
    doc_base is the number of the call's first document in the corpus; documents shorter than max(min_tokens, 1) or
    -- max_tokens > 0 -- longer than max_tokens stay as they are.  The rule: include/mbpe.h, mbpe_fim_spec."""
    return FimSpec(dropout_threshold(rate), dropout_threshold(spm_rate), int(seed) & 0xFFFFFFFFFFFFFFFF,
                   int(doc_base) & 0xFFFFFFFFFFFFFFFF, pre_id, suf_id, mid_id, min_tokens, max_tokens)


def fim_plan(doc_tok_off, spec):
    """mbpe_fim_plan (host only): what the transform does to documents of these token offsets -> (doc_tok_off after it
    [n_docs + 1], mode uint8[n_docs] (FIM_NONE / FIM_PSM / FIM_SPM), cuts uint64[n_docs, 2] = (a, b))."""
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    n_docs = len(off) - 1
    new_off = np.zeros(n_docs + 1, dtype=np.uint64)
    mode = np.zeros(max(n_docs, 1), dtype=np.uint8)
    cuts = np.zeros((max(n_docs, 1), 2), dtype=np.uint64)
    _check(lib().mbpe_fim_plan(off.ctypes.data, n_docs, ctypes.byref(spec), new_off.ctypes.data, mode.ctypes.data,
                               cuts.ctypes.data))
    return new_off, mode[:n_docs], cuts[:n_docs]


def fim_tokens(tokens, doc_tok_off, spec, device=0, tokens_ptr=None, n_tokens=None, token_bits=None, out_ptr=None,
               cap=0):
    """mbpe_fim_tokens: the fill-in-the-middle transform of a flat token array (uint16 or uint32) whose document i is
    tokens[doc_tok_off[i]:doc_tok_off[i + 1]] -> (tokens of the same dtype, doc_tok_off after it): what pack_* and
    Decoder.decode_batch take.  Device memory: tokens_ptr= / n_tokens= / token_bits= name the tokens there instead of
    `tokens`; with out_ptr= (room for cap tokens) the tokens are written there and (token count, doc_tok_off) is
    returned."""
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    if tokens_ptr is None:
        t = np.ascontiguousarray(tokens)
        if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            t = t.astype(np.uint32)
        t = t.reshape(-1)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    new_off = np.zeros(len(off), dtype=np.uint64)
    n = ctypes.c_uint64()
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    if out_ptr is not None:
        _check(lib().mbpe_fim_tokens(*head, _ptr(out_ptr), cap, 1, new_off.ctypes.data, ctypes.byref(n)))
        return n.value, new_off
    _check(lib().mbpe_fim_tokens(*head, None, 0, 0, new_off.ctypes.data, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=_ID_DTYPES[token_bits])
    _check(lib().mbpe_fim_tokens(*head, out.ctypes.data, n.value, 0, new_off.ctypes.data, ctypes.byref(n)))
    return out[:n.value], new_off


def fim_kernel_ms():
    """Device time of the kernels of this thread's latest fim_tokens (mbpe_fim_kernel_ms)."""
    ms = ctypes.c_float()
    _check(lib().mbpe_fim_kernel_ms(ctypes.byref(ms)))
    return ms.value


def denoise_spec(density=0.15, mean_span=3.0, sentinel_id=None, n_sentinels=100, sentinel_down=True, segment_tokens=0,
                 min_tokens=0, seed=0, doc_base=0):
    """A DenoiseSpec from T5's terms: `density` of every unit's tokens become noise, in runs of mean_span tokens on
    average; run j is replaced by the sentinel sentinel_id - j (sentinel_down, T5's <extra_id_j>) or sentinel_id + j,
    and no unit gets more than n_sentinels runs.  segment_tokens > 0 cuts every document into units of that many tokens
    first (denoise_segment_for() finds the number that fills two sequence lengths); units shorter than
    max(min_tokens, 2) stay as they are.  seed picks the epoch's draw, doc_base is the number of the call's first
    document in the corpus.  The rule: include/mbpe.h, mbpe_denoise_spec."""
    if sentinel_id is None:
        raise ValueError("sentinel_id is required: the id of the first sentinel")
    q8 = int(round(float(mean_span) * 256))
    return DenoiseSpec(dropout_threshold(density), int(seed) & 0xFFFFFFFFFFFFFFFF, int(doc_base) & 0xFFFFFFFFFFFFFFFF,
                       q8, segment_tokens, min_tokens, sentinel_id, int(bool(sentinel_down)), n_sentinels)


def _denoise_counts(L, density, mean_q8, n_sentinels, min_tokens=0):
    """(N, S) of a unit of L tokens -- the closed forms of include/mbpe.h -- for a density threshold."""
    if density == 0 or L < max(min_tokens, 2):
        return 0, 0
    N = min(max((L * density + (1 << 31)) >> 32, 1), L - 1)
    S = (N * 256 + mean_q8 // 2) // mean_q8
    return N, max(1, min(S, N, L - N, n_sentinels))


def denoise_segment_for(enc_len, dec_len, density=0.15, mean_span=3.0, eos=True, n_sentinels=100):
    """The largest segment_tokens whose units all fit: the inputs of every unit of up to that many tokens (and eos)
    fit enc_len, and its targets (and eos) fit dec_len, by search over the closed-form counts.  T5's 512 / 114 at the
    defaults give 568.  0 if not even a unit of one token fits."""
    thr, q8, e = dropout_threshold(density), int(round(float(mean_span) * 256)), int(bool(eos))
    best = 0
    while True:
        L = best + 1
        N, S = _denoise_counts(L, thr, q8, n_sentinels)
        if L - N + S + e > enc_len or (N + S + e if S else 0) > dec_len or L >= 0xFFFFFFFF:
            return best
        best = L


def _flat_tokens(tokens, tokens_ptr, n_tokens, token_bits):
    """tokens (or a device pointer) as the C-ABI takes them -> (array kept alive, pointer, count, bits, on_device)."""
    if tokens_ptr is not None:
        return None, _ptr(tokens_ptr), n_tokens, token_bits, 1
    t = np.ascontiguousarray(tokens)
    if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
        t = t.astype(np.uint32)
    t = t.reshape(-1)
    return t, (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0


def denoise_plan(doc_tok_off, spec):
    """mbpe_denoise_plan (host only): what span corruption makes of documents of these token offsets -> (unit_in_off
    [n_units + 1], unit_tg_off [n_units + 1], unit_doc [n_units]): the units' offsets into the inputs and into the
    targets, and every unit's document."""
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    n = ctypes.c_uint64()
    _check(lib().mbpe_denoise_plan(off.ctypes.data, len(off) - 1, ctypes.byref(spec), ctypes.byref(n), None, None, None, 0))
    in_off, tg_off = np.zeros(n.value + 1, dtype=np.uint64), np.zeros(n.value + 1, dtype=np.uint64)
    unit_doc = np.zeros(max(n.value, 1), dtype=np.uint64)
    _check(lib().mbpe_denoise_plan(off.ctypes.data, len(off) - 1, ctypes.byref(spec), ctypes.byref(n), in_off.ctypes.data,
                                   tg_off.ctypes.data, unit_doc.ctypes.data, n.value))
    return in_off, tg_off, unit_doc[:n.value]


def denoise_tokens(tokens, doc_tok_off, spec, device=0, tokens_ptr=None, n_tokens=None, token_bits=None, in_ptr=None,
                   cap_in=0, tg_ptr=None, cap_tg=0):
    """mbpe_denoise_tokens: span corruption of a flat token array (uint16 or uint32) whose document i is
    tokens[doc_tok_off[i]:doc_tok_off[i + 1]] -> (inputs, targets, unit_in_off, unit_tg_off, unit_doc): two flat arrays
    of the same dtype, one document ("unit") per row-to-be in each, which pack_* and Decoder.decode_batch take with
    their offsets.  Device memory: tokens_ptr= / n_tokens= / token_bits= name the tokens there instead of `tokens`; with
    in_ptr= and tg_ptr= (room for cap_in / cap_tg ids) the streams are written there and (n_in, n_tg, unit_in_off,
    unit_tg_off, unit_doc) is returned."""
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    keep, tp, n_tokens, token_bits, on_dev = _flat_tokens(tokens, tokens_ptr, n_tokens, token_bits)
    nu, ni, nt = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    tail = (ctypes.byref(nu), ctypes.byref(ni), ctypes.byref(nt))
    fn = lib().mbpe_denoise_tokens
    _check(fn(*head, None, 0, None, 0, 0, None, None, None, 0, *tail))
    in_off, tg_off = np.zeros(nu.value + 1, dtype=np.uint64), np.zeros(nu.value + 1, dtype=np.uint64)
    unit_doc = np.zeros(max(nu.value, 1), dtype=np.uint64)
    units = (in_off.ctypes.data, tg_off.ctypes.data, unit_doc.ctypes.data, nu.value)
    if in_ptr is not None:
        rc = fn(*head, _ptr(in_ptr), cap_in, _ptr(tg_ptr), cap_tg, 1, *units, *tail)
        _check(rc)
        return ni.value, nt.value, in_off, tg_off, unit_doc[:nu.value]
    inp = np.zeros(max(ni.value, 1), dtype=_ID_DTYPES[token_bits])
    tgt = np.zeros(max(nt.value, 1), dtype=_ID_DTYPES[token_bits])
    _check(fn(*head, inp.ctypes.data, ni.value, tgt.ctypes.data, nt.value, 0, *units, *tail))
    return inp[:ni.value], tgt[:nt.value], in_off, tg_off, unit_doc[:nu.value]


def denoise_kernel_ms():
    """Device time of the kernels of this thread's latest denoise_tokens (mbpe_denoise_kernel_ms)."""
    ms = ctypes.c_float()
    _check(lib().mbpe_denoise_kernel_ms(ctypes.byref(ms)))
    return ms.value


_DENOISE_PTRS = ("enc_ids", "enc_len", "dec_ids", "dec_len", "dec_labels", "row_doc")


def _denoise_specs(enc_len, dec_len, out_bits, pad_id, eos_id, decoder_start_id):
    """The two PADDED specs of a denoise batch: the encoder side ends in eos, the decoder side begins with the decoder
    start id and ends in eos (either None: none)."""
    return (pack_spec(enc_len, "padded", out_bits, pad_id, None, eos_id),
            pack_spec(dec_len, "padded", out_bits, pad_id, decoder_start_id, eos_id))


def _denoise_batch(call, n_docs, dn, enc_spec, dec_spec, ignore_label, ptrs, cap_rows, labels, row_doc):
    """One denoise batch call.  call(batch_ref, cap_rows, on_device) -> (rc, n_rows, n_tokens).  ptrs: a dict of device
    pointers by the names of mbpe_denoise_batch -> (n_rows, n_tokens); None -> (dict of numpy arrays, n_tokens)."""
    if ptrs is not None:
        unknown = set(ptrs) - set(_DENOISE_PTRS)
        if unknown:
            raise ValueError("unknown outputs: %s" % sorted(unknown))
        b = DenoiseBatch(*[ptrs.get(k) or None for k in _DENOISE_PTRS], int(ignore_label))
        rc, n_rows, n_tok = call(ctypes.byref(b), cap_rows or 0, 1)
        return rc, n_rows, n_tok
    if dn.segment_tokens == 0:
        n_rows = n_docs                               # known without a query
    else:
        rc, n_rows, n_tok = call(ctypes.byref(DenoiseBatch(None, None, None, None, None, None, int(ignore_label))), 0, 0)
        _check(rc)
    enc_ids, enc_n = _matrix(n_rows, enc_spec)
    dec_ids, dec_n = _matrix(n_rows, dec_spec)
    lab = np.zeros((n_rows, dec_spec.seq_len), dtype=_LABEL_DTYPES[dec_spec.out_bits]) if labels else None
    rd = np.zeros(n_rows, dtype=np.uint32) if row_doc else None
    out = {"enc_ids": enc_ids, "enc_len": enc_n, "dec_ids": dec_ids, "dec_len": dec_n}
    if labels:
        out["dec_labels"] = lab
    if row_doc:
        out["row_doc"] = rd
    n_tok = 0
    if n_rows:
        b = DenoiseBatch(enc_ids.ctypes.data, enc_n.ctypes.data, dec_ids.ctypes.data, dec_n.ctypes.data,
                         lab.ctypes.data if labels else None, rd.ctypes.data if row_doc else None, int(ignore_label))
        rc, _, n_tok = call(ctypes.byref(b), n_rows, 0)
        _check(rc)
    return 0, out, n_tok


def mlm_spec(rate, mask_id, vocab_n, mask_share=0.8, random_share=0.1, seed=0, doc_base=0, whole_word=False, protect=()):
    """An MlmSpec from probabilities: a token (with whole_word: a word) is selected with probability `rate`; a selected
    token becomes mask_id with probability mask_share, a random id below vocab_n with probability random_share, and
    stays otherwise -- a target either way.  seed picks the epoch's draw, doc_base is the number of the call's first
    document in the corpus; protect: up to 8 ids that are never selected (bos, eos, separators).  Random ids may be
    special ids unless vocab_n excludes them.  The rule: include/mbpe.h, mbpe_mlm_spec."""
    protect = [int(p) for p in protect]
    if len(protect) > 8:
        raise MbpeError(ERR_ARG, "mlm_spec: more than 8 protected ids")
    # (shares that sum to more than 1 give thresholds that sum to more than 2^32, which the library refuses)
    return MlmSpec(dropout_threshold(rate), dropout_threshold(mask_share), dropout_threshold(random_share),
                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(doc_base) & 0xFFFFFFFFFFFFFFFF, mask_id, vocab_n,
                   int(bool(whole_word)), len(protect), (ctypes.c_uint32 * 8)(*protect))


def _mlm_host_tokens(tokens, word_ends):
    t = np.ascontiguousarray(tokens)
    if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
        t = t.astype(np.uint32)
    t = t.reshape(-1)
    if word_ends is not None:
        if t.dtype != np.dtype(np.uint32):
            raise MbpeError(ERR_ARG, "word_ends go into bit 31 of 32-bit tokens: 16-bit tokens have no room for them")
        w = np.ascontiguousarray(word_ends, dtype=bool).reshape(-1)
        if len(w) != len(t):
            raise ValueError("word_ends must have one entry per token")
        t = t | (w.astype(np.uint32) << np.uint32(31))
    return t


def mlm_plan(tokens, doc_tok_off, spec, word_ends=None):
    """mbpe_mlm_plan (host only): the rule over a flat token array (uint16 or uint32; bit 31 of a uint32 token, or
    word_ends, marks the last token of a word) -> (tokens after it, same dtype; targets uint32, NO_TOKEN = none)."""
    t = _mlm_host_tokens(tokens, word_ends)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    out, tgt = np.zeros(max(len(t), 1), dtype=t.dtype), np.zeros(max(len(t), 1), dtype=np.uint32)
    _check(lib().mbpe_mlm_plan(t.ctypes.data if len(t) else None, len(t), t.dtype.itemsize * 8, off.ctypes.data,
                               len(off) - 1, ctypes.byref(spec), out.ctypes.data, tgt.ctypes.data))
    return out[:len(t)], tgt[:len(t)]


def mlm_tokens(tokens, doc_tok_off, spec, word_ends=None, device=0, tokens_ptr=None, n_tokens=None, token_bits=None,
               out_ptr=None, targets_ptr=None):
    """mbpe_mlm_tokens: masked-LM corruption of a flat token array (uint16 or uint32) whose document i is
    tokens[doc_tok_off[i]:doc_tok_off[i + 1]] -> (tokens of the same dtype, targets uint32 with NO_TOKEN where a token
    is no target): what pack_tokens_aux, pack_windows and pack_fit take as tokens and label_tokens=.  whole_word needs
    the word ends: bit 31 of uint32 tokens, or word_ends= (a bool per token), which is ORed into it.  Device memory:
    tokens_ptr= / n_tokens= / token_bits= name the tokens there instead of `tokens`; with out_ptr= (and targets_ptr=,
    or None) the results are written there and None is returned."""
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    if tokens_ptr is None:
        t = _mlm_host_tokens(tokens, word_ends)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    if out_ptr is not None:
        _check(lib().mbpe_mlm_tokens(*head, _ptr(out_ptr), _ptr(targets_ptr), 1))
        return None
    out = np.zeros(max(n_tokens, 1), dtype=_ID_DTYPES[token_bits])
    tgt = np.zeros(max(n_tokens, 1), dtype=np.uint32)
    _check(lib().mbpe_mlm_tokens(*head, out.ctypes.data, tgt.ctypes.data, 0))
    return out[:n_tokens], tgt[:n_tokens]


def mlm_kernel_ms():
    """Device time of the kernels of this thread's latest mlm_tokens (mbpe_mlm_kernel_ms)."""
    ms = ctypes.c_float()
    _check(lib().mbpe_mlm_kernel_ms(ctypes.byref(ms)))
    return ms.value


def _fim_info(fn, handle):
    n = ctypes.c_uint64()
    _check(fn(handle, None, None, 0, ctypes.byref(n)))
    mode = np.zeros(max(n.value, 1), dtype=np.uint8)
    cuts = np.zeros((max(n.value, 1), 2), dtype=np.uint64)
    _check(fn(handle, mode.ctypes.data, cuts.ctypes.data, n.value, ctypes.byref(n)))
    return mode[:n.value], cuts[:n.value]


def token_counts(tokens, n_ids, device=0, tokens_ptr=None, n_tokens=None, token_bits=None, out_ptr=None):
    """mbpe_token_counts: how often every id below n_ids occurs in a token array (uint16, or uint32 whose bit 31 is
    ignored) -> (counts uint64[n_ids], n_other), n_other counting the ids at or beyond n_ids.  Device memory:
    tokens_ptr= / n_tokens= / token_bits= name the tokens there instead of `tokens`; with out_ptr= (room for n_ids
    uint64) the table is written there and only n_other is returned."""
    if tokens_ptr is None:
        t = np.ascontiguousarray(tokens)
        if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            t = t.astype(np.uint32)
        t = t.reshape(-1)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    other = ctypes.c_uint64()
    if out_ptr is not None:
        _check(lib().mbpe_token_counts(device, tp, n_tokens, token_bits, on_dev, _ptr(out_ptr), n_ids, 1, ctypes.byref(other)))
        return other.value
    # (the library checks n_ids before it writes: the array only has to exist for a valid one)
    out = np.zeros(n_ids if 0 < n_ids <= (1 << 25) else 1, dtype=np.uint64)
    _check(lib().mbpe_token_counts(device, tp, n_tokens, token_bits, on_dev, out.ctypes.data, n_ids, 0, ctypes.byref(other)))
    return out, other.value


def token_counts_kernel_ms():
    """Device time of the histogram kernel of this thread's latest token_counts (mbpe_token_counts_kernel_ms)."""
    ms = ctypes.c_float()
    _check(lib().mbpe_token_counts_kernel_ms(ctypes.byref(ms)))
    return ms.value


def pack_cu_seqlens(doc_tok_off, seq_len, bos_id=None, eos_id=None):
    """mbpe_pack_cu_seqlens: the boundaries of the runs of equal (row, segment) in the flattened MBPE_PACK_PACKED matrix
    of these documents -> (int32 array of n_seqs + 1 entries, max_seqlen).  Host arithmetic alone: needs no device."""
    spec = pack_spec(seq_len, "packed", 32, 0, bos_id, eos_id)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    n_seqs, longest = ctypes.c_uint64(), ctypes.c_uint32()
    head = (off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    _check(lib().mbpe_pack_cu_seqlens(*head, None, 0, ctypes.byref(n_seqs), ctypes.byref(longest)))
    cu = np.zeros(n_seqs.value + 1, dtype=np.int32)
    _check(lib().mbpe_pack_cu_seqlens(*head, cu.ctypes.data, n_seqs.value, ctypes.byref(n_seqs), ctypes.byref(longest)))
    return cu, longest.value


def _label_call(fn, fn_labels, label_tokens, on_dev, n_tokens):
    """label_tokens= of the pack calls -> (the entry point, its trailing arguments, what keeps them alive)"""
    if label_tokens is None:
        return fn, (), None
    if on_dev:
        return fn_labels, (_ptr(int(label_tokens)),), None
    a = np.ascontiguousarray(label_tokens, dtype=np.uint32).reshape(-1)
    if len(a) != n_tokens:
        raise ValueError("label_tokens must have one entry per token")
    return fn_labels, (a.ctypes.data if len(a) else None,), a


class _AuxCall:
    """What the three *_aux calls share: the mbpe_pack_aux of a call and the dict it returns."""

    def __init__(self, spec, labels, positions, segments, cu_seqlens, ignore_label):
        self.spec, self.want, self.cu = spec, (labels, positions, segments), cu_seqlens
        self.ignore = int(ignore_label)

    def device(self, labels_ptr, pos_ptr, seg_ptr):
        return PackAux(labels_ptr or None, pos_ptr or None, seg_ptr or None, self.ignore)

    def host(self, n_rows):
        """-> (PackAux, its arrays by name) for n_rows rows in host memory."""
        shape = (n_rows, self.spec.seq_len)
        dtypes = (("labels", _LABEL_DTYPES[self.spec.out_bits]), ("positions", np.uint32), ("segments", np.uint32))
        arrays = {name: np.zeros(shape, dtype=dt) for (name, dt), w in zip(dtypes, self.want) if w}
        ptr = lambda name: arrays[name].ctypes.data if name in arrays and arrays[name].size else None
        return PackAux(ptr("labels"), ptr("positions"), ptr("segments"), self.ignore), arrays

    def result(self, ids, lengths, arrays, doc_tok_off):
        out = {"ids": ids, "lengths": lengths}
        out.update(arrays)
        if self.cu:
            out["cu_seqlens"], out["max_seqlen"] = self.cu_seqlens(doc_tok_off)
        return out

    def cu_seqlens(self, doc_tok_off):
        none = lambda t: None if t == NO_TOKEN else t
        return pack_cu_seqlens(doc_tok_off, self.spec.seq_len, none(self.spec.bos_id), none(self.spec.eos_id))


def pack_tokens_aux(tokens, doc_tok_off, seq_len, layout="padded", out_bits=32, pad_id=0, bos_id=None, eos_id=None,
                    pad_left=False, trunc_left=False, device=0, tokens_ptr=None, n_tokens=None, token_bits=None,
                    out_ptr=None, len_ptr=None, cap_rows=None, labels=False, positions=False, segments=False,
                    cu_seqlens=False, ignore_label=-100, labels_ptr=None, pos_ptr=None, seg_ptr=None, label_tokens=None):
    """mbpe_pack_tokens_aux: pack_tokens plus what a training step needs, from one kernel -> a dict with "ids",
    "lengths" and whichever of "labels" (next-token targets that never cross a document; ignore_label elsewhere; int32
    / int64, uint16 for out_bits 16), "positions" (uint32, restarting at every document), "segments" (uint32, document
    number + 1, 0 = pad) and "cu_seqlens" with "max_seqlen" (layout "packed" only) were asked for.
    With out_ptr= the matrices go to device memory at out_ptr / len_ptr / labels_ptr / pos_ptr / seg_ptr (each 16-byte
    aligned; None = not wanted) and the row count is returned -- (row count, cu_seqlens, max_seqlen) with
    cu_seqlens=True.
    label_tokens= (here, in pack_windows and in pack_fit; mbpe_pack_tokens_aux_labels and its kin): a uint32 target per
    token, on the side of the tokens (an array, or a device address with tokens_ptr=) -- the targets of mlm_tokens.  The
    labels are then these targets in the cells of their tokens and ignore_label wherever the target is NO_TOKEN and in
    bos, eos and pad cells; everything else is as without."""
    spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
    call = _AuxCall(spec, labels, positions, segments, cu_seqlens, ignore_label)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    if tokens_ptr is None:
        t = np.ascontiguousarray(tokens)
        if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            t = t.astype(np.uint32)
        t = t.reshape(-1)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    n_rows = ctypes.c_uint64()
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    fn, extra, _keep = _label_call(lib().mbpe_pack_tokens_aux, lib().mbpe_pack_tokens_aux_labels, label_tokens, on_dev,
                                   n_tokens)
    if out_ptr is not None:
        aux = call.device(labels_ptr, pos_ptr, seg_ptr)
        cu = call.cu_seqlens(off) if cu_seqlens else None
        _check(fn(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), ctypes.byref(n_rows), ctypes.byref(aux), *extra))
        return (n_rows.value,) + cu if cu_seqlens else n_rows.value
    aux = call.device(None, None, None)
    _check(fn(*head, None, 0, 0, None, ctypes.byref(n_rows), ctypes.byref(aux), *extra))
    ids, lengths = _matrix(n_rows.value, spec)
    aux, arrays = call.host(n_rows.value)
    if n_rows.value:
        _check(fn(*head, ids.ctypes.data, n_rows.value, 0, lengths.ctypes.data, ctypes.byref(n_rows), ctypes.byref(aux),
                  *extra))
    return call.result(ids, lengths, arrays, off)


class _WinCall(_AuxCall):
    """What the *_windows calls share: the mbpe_pack_aux and the mbpe_pack_window of a call, the query for the row
    count, and the dict it returns."""

    def __init__(self, spec, stride, score_once, labels, positions, segments, ignore_label, row_doc, row_tok0):
        super().__init__(spec, labels, positions, segments, False, ignore_label)
        self.stride, self.once, self.want_rows = int(stride), int(bool(score_once)), (row_doc, row_tok0)

    def window(self, row_doc_ptr=None, row_tok0_ptr=None):
        return PackWindow(self.stride, self.once, row_doc_ptr or None, row_tok0_ptr or None)

    def run(self, fn, head, tail, out_ptr, len_ptr, cap_rows, ptrs):
        """fn(*head, ids, cap_rows, on_device, len, *tail(n_rows), aux, ..., win): with out_ptr= into device memory ->
        the row count; else a query, host arrays of that size and the call -> the dict."""
        n_rows = ctypes.c_uint64()
        if out_ptr is not None:
            aux, win = self.device(*ptrs[:3]), self.window(*ptrs[3:])
            rc = fn(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail(n_rows, aux, win))
            self.n_rows = n_rows.value               # (reported also where a cap_rows too small is refused)
            _check(rc)
            return n_rows.value
        aux, win = self.device(None, None, None), self.window()
        _check(fn(*head, None, 0, 0, None, *tail(n_rows, aux, win)))
        n = n_rows.value
        ids, lengths = _matrix(n, self.spec)
        aux, arrays = self.host(n)
        if self.want_rows[0]:
            arrays["row_doc"] = np.zeros(n, dtype=np.uint32)
        if self.want_rows[1]:
            arrays["row_tok0"] = np.zeros(n, dtype=np.uint64)
        ptr = lambda name: arrays[name].ctypes.data if name in arrays and n else None
        win = self.window(ptr("row_doc"), ptr("row_tok0"))
        if n:
            _check(fn(*head, ids.ctypes.data, n, 0, lengths.ctypes.data, *tail(n_rows, aux, win)))
        return self.result(ids, lengths, arrays, None)


def pack_windows(tokens, doc_tok_off, seq_len, stride, score_once=False, out_bits=32, pad_id=0, bos_id=None, eos_id=None,
                 device=0, tokens_ptr=None, n_tokens=None, token_bits=None, out_ptr=None, len_ptr=None, cap_rows=None,
                 labels=False, positions=False, segments=False, ignore_label=-100, labels_ptr=None, pos_ptr=None,
                 seg_ptr=None, row_doc=False, row_tok0=False, row_doc_ptr=None, row_tok0_ptr=None, label_tokens=None):
    """mbpe_pack_windows: one document per row like pack_tokens_aux(layout="padded"), but a document longer than
    keep = seq_len - (bos) - (eos) tokens becomes several rows of its own, consecutive ones sharing `stride` tokens
    (window i holds tokens [i * (keep - stride), i * (keep - stride) + keep); bos in every row, eos in the last).
    Labels also cross the row end inside a document; score_once=True sets the labels of the shared cells of every
    later window to ignore_label, so that each target is scored once.  -> the dict of pack_tokens_aux plus "row_doc"
    (uint32: the row's document) and "row_tok0" (uint64: the index in the document of the row's first token) when
    asked for.  With out_ptr= the outputs go to device memory (row_doc_ptr= / row_tok0_ptr= beside the pointers of
    pack_tokens_aux) and the row count is returned."""
    spec = pack_spec(seq_len, "padded", out_bits, pad_id, bos_id, eos_id)
    call = _WinCall(spec, stride, score_once, labels, positions, segments, ignore_label, row_doc, row_tok0)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    if tokens_ptr is None:
        t = np.ascontiguousarray(tokens)
        if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            t = t.astype(np.uint32)
        t = t.reshape(-1)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    fn, extra, _keep = _label_call(lib().mbpe_pack_windows, lib().mbpe_pack_windows_labels, label_tokens, on_dev, n_tokens)
    tail = lambda n_rows, aux, win: (ctypes.byref(n_rows), ctypes.byref(aux), ctypes.byref(win)) + extra
    return call.run(fn, head, tail, out_ptr, len_ptr, cap_rows,
                    (labels_ptr, pos_ptr, seg_ptr, row_doc_ptr, row_tok0_ptr))


def _fit_spec(seq_len, out_bits=32, pad_id=0, bos_id=None, eos_id=None):
    return pack_spec(seq_len, "packed", out_bits, pad_id, bos_id, eos_id)


def pack_fit_plan(doc_tok_off, seq_len, bos_id=None, eos_id=None):
    """mbpe_pack_fit_plan: where best-fit packing puts documents of these token offsets into rows of seq_len -> a
    dict with "n_rows", "lengths" (uint32, the cells used per row), "doc_row" (uint64) and "doc_col" (uint32): the cell
    of the first element of every document's last piece (2^64 - 1 and 0 for a document without elements).  Host
    arithmetic alone: needs no device."""
    spec = _fit_spec(seq_len, bos_id=bos_id, eos_id=eos_id)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    n_docs = len(off) - 1
    n_rows = ctypes.c_uint64()
    head = (off.ctypes.data, n_docs, ctypes.byref(spec))
    # one plan, not a query and a plan: there are no more rows than pieces.  (A count beyond reason -- offsets that
    # descend wrap to one -- goes to the query, which refuses what the library refuses)
    T = np.diff(off) + np.uint64((bos_id is not None) + (eos_id is not None))
    cap = int((T // np.uint64(max(seq_len, 1))).sum() + np.count_nonzero(T)) if n_docs > 0 else 0
    if cap >> 32:
        _check(lib().mbpe_pack_fit_plan(*head, None, 0, ctypes.byref(n_rows), None, None))
        cap = n_rows.value
    lengths = np.zeros(cap, dtype=np.uint32)
    doc_row, doc_col = np.zeros(n_docs, dtype=np.uint64), np.zeros(n_docs, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if len(a) else None
    _check(lib().mbpe_pack_fit_plan(*head, ptr(lengths), len(lengths), ctypes.byref(n_rows), ptr(doc_row), ptr(doc_col)))
    return {"n_rows": n_rows.value, "lengths": lengths[:n_rows.value], "doc_row": doc_row, "doc_col": doc_col}


def pack_fit_cu_seqlens(doc_tok_off, seq_len, bos_id=None, eos_id=None):
    """mbpe_pack_fit_cu_seqlens: the boundaries of the runs of equal (row, segment) in the flattened matrix of pack_fit,
    pad runs included, from 0 to n_rows * seq_len -> (int32 array of n_seqs + 1 entries, max_seqlen).  Host arithmetic
    alone: needs no device."""
    spec = _fit_spec(seq_len, bos_id=bos_id, eos_id=eos_id)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    n_seqs, longest = ctypes.c_uint64(), ctypes.c_uint32()
    head = (off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    _check(lib().mbpe_pack_fit_cu_seqlens(*head, None, 0, ctypes.byref(n_seqs), ctypes.byref(longest)))
    cu = np.zeros(n_seqs.value + 1, dtype=np.int32)
    _check(lib().mbpe_pack_fit_cu_seqlens(*head, cu.ctypes.data, n_seqs.value, ctypes.byref(n_seqs), ctypes.byref(longest)))
    return cu, longest.value


class _FitCall(_AuxCall):
    """What the *_fit calls share: the mbpe_pack_aux and the mbpe_pack_fit of a call, the query for the row count, and
    the dict it returns."""

    def __init__(self, spec, labels, positions, segments, cu_seqlens, ignore_label, doc_row, doc_col):
        super().__init__(spec, labels, positions, segments, cu_seqlens, ignore_label)
        self.want_docs = (doc_row, doc_col)

    def cu_seqlens(self, doc_tok_off):
        none = lambda t: None if t == NO_TOKEN else t
        return pack_fit_cu_seqlens(doc_tok_off, self.spec.seq_len, none(self.spec.bos_id), none(self.spec.eos_id))

    def run(self, fn, head, tail, n_docs, doc_tok_off, out_ptr, len_ptr, cap_rows, ptrs):
        """fn(*head, ids, cap_rows, on_device, len, *tail(n_rows, aux, fit)): with out_ptr= into device memory -> the
        row count (with cu_seqlens: and the list and max_seqlen); else a query, host arrays of that size and the call
        -> the dict.  doc_tok_off(): the documents' token offsets once fn has run."""
        n_rows = ctypes.c_uint64()
        if out_ptr is not None:
            aux, fit = self.device(*ptrs[:3]), PackFit(ptrs[3] or None, ptrs[4] or None)
            rc = fn(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail(n_rows, aux, fit))
            self.n_rows = n_rows.value               # (reported also where a cap_rows too small is refused)
            _check(rc)
            return (n_rows.value,) + self.cu_seqlens(doc_tok_off()) if self.cu else n_rows.value
        aux, fit = self.device(None, None, None), PackFit(None, None)
        _check(fn(*head, None, 0, 0, None, *tail(n_rows, aux, fit)))
        n = n_rows.value
        ids, lengths = _matrix(n, self.spec)
        aux, arrays = self.host(n)
        if self.want_docs[0]:
            arrays["doc_row"] = np.zeros(n_docs, dtype=np.uint64)
        if self.want_docs[1]:
            arrays["doc_col"] = np.zeros(n_docs, dtype=np.uint32)
        ptr = lambda name: arrays[name].ctypes.data if name in arrays and n_docs else None
        fit = PackFit(ptr("doc_row"), ptr("doc_col"))
        if n or n_docs:
            # (no row, yet documents: doc_row says that they are empty; ids_out must not be NULL, which is the query)
            where = ids if n else np.zeros(1, dtype=ids.dtype)
            _check(fn(*head, where.ctypes.data, n, 0, lengths.ctypes.data if n else None, *tail(n_rows, aux, fit)))
        return self.result(ids, lengths, arrays, doc_tok_off())


def pack_fit(tokens, doc_tok_off, seq_len, out_bits=32, pad_id=0, bos_id=None, eos_id=None, device=0, tokens_ptr=None,
             n_tokens=None, token_bits=None, out_ptr=None, len_ptr=None, cap_rows=None, labels=False, positions=False,
             segments=False, cu_seqlens=False, ignore_label=-100, labels_ptr=None, pos_ptr=None, seg_ptr=None,
             doc_row=False, doc_col=False, doc_row_ptr=None, doc_col_ptr=None, label_tokens=None):
    """mbpe_pack_fit: best-fit packing.  Every document [bos] doc [eos] stays whole and shares its row with others;
    only a document longer than seq_len is cut, into full rows of its own and one tail.  The pieces are placed by size
    descending into the row with the least room that still holds them, so padding stays small and lies at the right
    end of a row.  Labels, positions and segments as for layout "packed" of pack_tokens_aux: use them, or cu_seqlens
    (pad runs are sequences of their own there), to keep attention inside a document.  -> the dict of pack_tokens_aux
    plus "doc_row" (uint64) and "doc_col" (uint32) when asked for: the cell of the first element of each document's
    last piece.  With out_ptr= the outputs go to device memory (doc_row_ptr= / doc_col_ptr= beside the pointers of
    pack_tokens_aux) and the row count is returned -- (row count, cu_seqlens, max_seqlen) with cu_seqlens=True."""
    spec = _fit_spec(seq_len, out_bits, pad_id, bos_id, eos_id)
    call = _FitCall(spec, labels, positions, segments, cu_seqlens, ignore_label, doc_row, doc_col)
    off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
    if tokens_ptr is None:
        t = np.ascontiguousarray(tokens)
        if t.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            t = t.astype(np.uint32)
        t = t.reshape(-1)
        tp, n_tokens, token_bits, on_dev = (t.ctypes.data if len(t) else None), len(t), t.dtype.itemsize * 8, 0
    else:
        tp, on_dev = _ptr(tokens_ptr), 1
    head = (device, tp, n_tokens, token_bits, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(spec))
    fn, extra, _keep = _label_call(lib().mbpe_pack_fit, lib().mbpe_pack_fit_labels, label_tokens, on_dev, n_tokens)
    tail = lambda n_rows, aux, fit: (ctypes.byref(n_rows), ctypes.byref(aux), ctypes.byref(fit)) + extra
    return call.run(fn, head, tail, len(off) - 1, lambda: off, out_ptr, len_ptr, cap_rows,
                    (labels_ptr, pos_ptr, seg_ptr, doc_row_ptr, doc_col_ptr))


def unpack_tokens(ids, lengths, dtype=np.uint32, device=0, ids_ptr=None, len_ptr=None, shape=None, id_bits=None,
                  out_ptr=None, cap=0):
    """mbpe_unpack_tokens: a right-padded matrix ids [n_rows, seq_len] (uint16 / uint32 / uint64) and its lengths ->
    (tokens of dtype uint32 or uint16, doc_tok_off [n_rows + 1]).  Device memory: ids_ptr= / len_ptr= / shape= /
    id_bits= name the matrix there; with out_ptr= (room for cap tokens) the tokens are written there and (token count,
    doc_tok_off) is returned -- what Decoder.decode_batch_device takes."""
    dtype = np.dtype(dtype)
    if ids_ptr is None:
        m = np.ascontiguousarray(ids)
        if m.dtype not in (np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64)):
            m = m.astype(np.uint32)
        n_rows, seq_len = m.shape
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        ip, lp, id_bits, on_dev = (m.ctypes.data if m.size else None), (ln.ctypes.data if len(ln) else None), \
            m.dtype.itemsize * 8, 0
    else:
        (n_rows, seq_len), ip, lp, on_dev = shape, _ptr(ids_ptr), _ptr(len_ptr), 1
    off = np.zeros(n_rows + 1, dtype=np.uint64)
    n = ctypes.c_uint64()
    head = (device, ip, n_rows, seq_len, id_bits, on_dev, lp)
    if out_ptr is not None:
        _check(lib().mbpe_unpack_tokens(*head, _ptr(out_ptr), cap, dtype.itemsize * 8, 1, off.ctypes.data,
                                        ctypes.byref(n)))
        return n.value, off
    _check(lib().mbpe_unpack_tokens(*head, None, 0, dtype.itemsize * 8, 0, off.ctypes.data, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=dtype)
    _check(lib().mbpe_unpack_tokens(*head, out.ctypes.data, n.value, dtype.itemsize * 8, 0, off.ctypes.data,
                                    ctypes.byref(n)))
    return out[:n.value], off


def pack_kernel_ms():
    """Device time of this thread's latest pack_tokens / unpack_tokens kernel (mbpe_pack_kernel_ms)."""
    ms = ctypes.c_float()
    _check(lib().mbpe_pack_kernel_ms(ctypes.byref(ms)))
    return ms.value


SINGLE = np.dtype([("start", np.uint64), ("len", np.uint64), ("id", np.uint32), ("pad", np.uint32)])   # mbpe_single
SPLIT_RAW = 0xFFFFFFFF      # MBPE_SPLIT_RAW: the name of a range that is a NUL-led part


def dropout_threshold(p):
    """A dropout probability in [0, 1] -> the threshold floor(p * 2^32) of mbpe_encoder_set_dropout
    (mbpe_dropout_threshold; NaN or a value outside [0, 1] raises the library's error)."""
    t = ctypes.c_uint64()
    _check(lib().mbpe_dropout_threshold(float(p), ctypes.byref(t)))
    return t.value


def _singles(rows):
    """rows (start, len, id) -> an array of mbpe_single."""
    out = np.zeros(0 if rows is None else len(rows), dtype=SINGLE)
    for k, (a, n, i) in enumerate([] if rows is None else rows):
        out[k] = (a, n, i, 0)
    return out


class Encoder:
    """One mbpe_encoder: internal_encode (Tokenizer.h:325-377) on a HIP device with the lookup table, the stream and
    the work buffers kept between calls."""

    def __init__(self, merges, device=0, rank_order=False, dropout=0.0, seed=0, dedup=False, count_ids=None):
        """count_ids: the option "count_ids" from the start: the table of count() has max(256 + n_merges, count_ids) bins.
        rank_order: the option "rank_order" from the start (set_option changes it between calls).
        dropout, seed: BPE-dropout from the start (set_dropout changes it between calls); needs rank_order.
        dedup: the option "dedup" from the start: every call dedups its chunks on the device, encodes the distinct
        ones and expands (the same results; dropout and byte offsets raise MbpeError(ERR_ARG) while it is on)."""
        self._h = ctypes.c_void_p()
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
        _check(lib().mbpe_encoder_create(device, m.ctypes.data if len(m) else None, len(m), ctypes.byref(self._h)))
        self.n_passes = 0
        self.n_tokens = 0
        if rank_order:
            self.set_option("rank_order", 1)
        if dropout or seed:
            self.set_dropout(dropout, seed)
        if dedup:
            self.set_option("dedup", 1)
        if count_ids is not None:
            self.set_option("count_ids", count_ids)

    def close(self):
        if self._h:
            lib().mbpe_encoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        _check(lib().mbpe_encoder_set_option(self._h, name.encode(), int(value)))

    def set_dropout(self, p, seed=0):
        """BPE-dropout for the calls that follow (mbpe_encoder_set_dropout): a merge instance -- (byte start of the
        pair's left token in the call's text, merged id) -- is skipped with probability p, decided by a hash of
        (seed, position, id).  Rank order only: an encode call with p > 0 and the greedy order raises MbpeError(ERR_ARG).
        p = 0 is plain rank order, p = 1 leaves the bytes."""
        _check(lib().mbpe_encoder_set_dropout(self._h, dropout_threshold(p), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_fim(self, spec):
        """Fill-in-the-middle for the batch calls that follow (mbpe_encoder_set_fim): a FimSpec (fim_spec()), or None
        to turn it off.  The stage runs between the encode and the pack kernel of encode_batch, _aux, _windows, _fit and
        their endmask forms; the flat calls and count() are unaffected.  doc_tok_off of those calls is the one after
        the transform."""
        _check(lib().mbpe_encoder_set_fim(self._h, None if spec is None else ctypes.byref(spec)))

    def set_mlm(self, spec):
        """Masked-LM corruption for the batch calls that follow (mbpe_encoder_set_mlm): an MlmSpec (mlm_spec()), or None
        to turn it off.  The matrices hold the corrupted ids and "labels" the targets."""
        _check(lib().mbpe_encoder_set_mlm(self._h, None if spec is None else ctypes.byref(spec)))

    def fim_info(self):
        """The plan of the latest batch call (mbpe_encoder_fim_info) -> (mode uint8[n_docs], cuts uint64[n_docs, 2]);
        all zero where the stage was off."""
        return _fim_info(lib().mbpe_encoder_fim_info, self._h)

    def encode(self, data, chunk_off=None, offsets=False, dtype=np.uint32, byte_off=False, text_ptr=None, n_bytes=None,
               cap=None):
        """Host text -> host tokens of dtype uint32 or uint16, or (tokens, chunk_tok_off) with offsets=True: the
        tokens of chunk c are tokens[chunk_tok_off[c]:chunk_tok_off[c + 1]].  The passes made: self.n_passes.
        byte_off=True (mbpe_encoder_encode_byteoff) appends tok_byte_off to the result, n + 1 uint64 offsets: token j
        stands for data[tok_byte_off[j]:tok_byte_off[j + 1]].
        text_ptr= / n_bytes= name a text in device memory instead of `data`.  cap= the room of the host array in tokens
        (default: n_bytes, which always suffices).  The count the library reported, also when it refused a cap that is
        too small: self.n_out."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint32), np.dtype(np.uint16)):
            raise ValueError("dtype must be uint32 or uint16")
        if text_ptr is None:
            text = _u8(data)
            tp, n_bytes, on_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            tp, on_dev = _ptr(text_ptr), 1
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        n_chunks = 1 if off is None else len(off) - 1
        room = n_bytes if cap is None else cap
        out = np.zeros(max(room, 1), dtype=dtype)
        tok_off = np.zeros(n_chunks + 1, dtype=np.uint64) if offsets else None
        n, passes = ctypes.c_uint64(), ctypes.c_uint32()
        head = (self._h, tp, n_bytes, on_dev, None if off is None else off.ctypes.data, 0 if off is None else n_chunks,
                out.ctypes.data, room if cap is not None else len(out), dtype.itemsize * 8, 0)
        tail = (None if tok_off is None else tok_off.ctypes.data, ctypes.byref(n), ctypes.byref(passes))
        if byte_off:
            boff = np.zeros(len(out) + 1, dtype=np.uint64)
            rc = lib().mbpe_encoder_encode_byteoff(*head, boff.ctypes.data, *tail)
        else:
            rc = lib().mbpe_encoder_encode(*head, *tail)
        self.n_out = n.value
        _check(rc)
        self.n_passes = passes.value
        tokens = out[:n.value].copy()
        res = (tokens, tok_off) if offsets else (tokens,)
        if byte_off:
            res += (boff[:n.value + 1].copy(),)
        return res if len(res) > 1 else res[0]

    def encode_device(self, text_ptr, n_bytes, chunk_off, out_ptr, cap, token_bits=32, offsets=False, byte_off_ptr=None,
                      text_on_device=True):
        """n_bytes of text in device memory at text_ptr (e.g. a torch tensor's data_ptr(); read in place) -> tokens in
        device memory at out_ptr (0: query; room for cap tokens of token_bits bits; 32: bit 31 = chunk end, 16: plain
        ids) -> token count, or (count, chunk_tok_off) with offsets=True.  byte_off_ptr: device memory for cap + 1
        uint64, filled with the count + 1 token byte offsets (mbpe_encoder_encode_byteoff).  text_on_device=False:
        text_ptr is an address in host memory.  The count the library reported, also when it refused: self.n_out."""
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        n_chunks = 1 if off is None else len(off) - 1
        tok_off = np.zeros(n_chunks + 1, dtype=np.uint64) if offsets else None
        n, passes = ctypes.c_uint64(), ctypes.c_uint32()
        head = (self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, n_bytes, int(bool(text_on_device)),
                None if off is None else off.ctypes.data, 0 if off is None else n_chunks,
                ctypes.c_void_p(out_ptr) if out_ptr else None, cap, token_bits, 1)
        tail = (None if tok_off is None else tok_off.ctypes.data, ctypes.byref(n), ctypes.byref(passes))
        if byte_off_ptr:
            rc = lib().mbpe_encoder_encode_byteoff(*head, ctypes.c_void_p(byte_off_ptr), *tail)
        else:
            rc = lib().mbpe_encoder_encode(*head, *tail)
        self.n_out = n.value
        _check(rc)
        self.n_passes = passes.value
        return (n.value, tok_off) if offsets else n.value

    def encode_batch(self, texts_or_buffer, chunk_off=None, doc_chunk_off=None, *, seq_len, layout="padded",
                     out_bits=32, pad_id=0, bos_id=None, eos_id=None, pad_left=False, trunc_left=False,
                     text_ptr=None, n_bytes=None, out_ptr=None, len_ptr=None, cap_rows=None):
        """Encode and pack in one device call (mbpe_encoder_encode_batch) -> (ids [n_rows, seq_len], lengths [n_rows]) as
        numpy arrays; the tokens encoded: self.n_tokens.
        texts_or_buffer: a list of texts, each one document and one chunk; or one buffer with chunk_off (as for
        encode) and doc_chunk_off, n_docs + 1 chunk indices: document i is the chunks doc_chunk_off[i] ..
        doc_chunk_off[i + 1] (None: every chunk a document).  text_ptr= / n_bytes= name a buffer in device memory
        instead.  With out_ptr= and len_ptr= (device memory for cap_rows rows, e.g. a torch tensor's data_ptr()) the
        matrix is written there and the row count is returned."""
        spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
        head, keep = self._batch_head(texts_or_buffer, chunk_off, doc_chunk_off, text_ptr, n_bytes, spec)
        docs = keep[-1]
        n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
        tail = (ctypes.byref(n_rows), ctypes.byref(n_tok))
        if out_ptr is not None:
            rc = lib().mbpe_encoder_encode_batch(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail)
            self.n_rows, self.n_tokens = n_rows.value, n_tok.value     # (also where a cap_rows too small is refused)
            _check(rc)
            return n_rows.value
        if spec.layout == PACK_PADDED:
            n_rows.value = len(docs) - 1              # known without a query
        else:
            _check(lib().mbpe_encoder_encode_batch(*head, None, 0, 0, None, *tail))
        ids, lengths = _matrix(n_rows.value, spec)
        _check(lib().mbpe_encoder_encode_batch(*head, ids.ctypes.data if ids.size else None, len(ids), 0,
                                               lengths.ctypes.data if len(ids) else None, *tail))
        self.n_tokens = n_tok.value
        return ids, lengths

    def _batch_head(self, texts_or_buffer, chunk_off, doc_chunk_off, text_ptr, n_bytes, spec):
        """The arguments of mbpe_encoder_encode_batch up to spec -> (tuple, the arrays it points into; the last of them
        the documents' chunk offsets)."""
        if text_ptr is None and isinstance(texts_or_buffer, (list, tuple)):
            parts = [bytes(_u8(t)) for t in texts_or_buffer]
            chunk_off = np.zeros(len(parts) + 1, dtype=np.uint64)
            if parts:
                chunk_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
            texts_or_buffer, doc_chunk_off = b"".join(parts), None
        text = None
        if text_ptr is None:
            text = _u8(texts_or_buffer)
            tp, n_bytes, on_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            tp, on_dev = _ptr(text_ptr), 1
        off = np.array([0, n_bytes], dtype=np.uint64) if chunk_off is None else \
            np.ascontiguousarray(chunk_off, dtype=np.uint64)
        docs = np.arange(len(off), dtype=np.uint64) if doc_chunk_off is None else \
            np.ascontiguousarray(doc_chunk_off, dtype=np.uint64)
        head = (self._h, tp, n_bytes, on_dev, off.ctypes.data, len(off) - 1, docs.ctypes.data, len(docs) - 1,
                ctypes.byref(spec))
        return head, (text, off, docs)

    def encode_batch_aux(self, texts_or_buffer, chunk_off=None, doc_chunk_off=None, *, seq_len, layout="padded",
                         out_bits=32, pad_id=0, bos_id=None, eos_id=None, pad_left=False, trunc_left=False,
                         text_ptr=None, n_bytes=None, out_ptr=None, len_ptr=None, cap_rows=None, labels=False,
                         positions=False, segments=False, cu_seqlens=False, ignore_label=-100, labels_ptr=None,
                         pos_ptr=None, seg_ptr=None):
        """encode_batch plus labels, positions, segments and cu_seqlens (mbpe_encoder_encode_batch_aux): the arguments
        of encode_batch and those of pack_tokens_aux, whose dict (or, with out_ptr=, row count) is returned.  The
        documents' token offsets of the call: self.doc_tok_off."""
        spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
        call = _AuxCall(spec, labels, positions, segments, cu_seqlens, ignore_label)
        head, keep = self._batch_head(texts_or_buffer, chunk_off, doc_chunk_off, text_ptr, n_bytes, spec)
        n_docs = len(keep[-1]) - 1
        n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
        doc_tok_off = np.zeros(n_docs + 1, dtype=np.uint64)
        tail = (ctypes.byref(n_rows), ctypes.byref(n_tok))
        if out_ptr is not None:
            aux = call.device(labels_ptr, pos_ptr, seg_ptr)
            rc = lib().mbpe_encoder_encode_batch_aux(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail,
                                                     ctypes.byref(aux), doc_tok_off.ctypes.data)
            self.n_rows, self.n_tokens, self.doc_tok_off = n_rows.value, n_tok.value, doc_tok_off
            _check(rc)
            return (n_rows.value,) + call.cu_seqlens(doc_tok_off) if cu_seqlens else n_rows.value
        if spec.layout == PACK_PADDED:
            n_rows.value = n_docs                     # known without a query
        else:
            aux = call.device(None, None, None)
            _check(lib().mbpe_encoder_encode_batch_aux(*head, None, 0, 0, None, *tail, ctypes.byref(aux), None))
        ids, lengths = _matrix(n_rows.value, spec)
        aux, arrays = call.host(n_rows.value)
        _check(lib().mbpe_encoder_encode_batch_aux(*head, ids.ctypes.data if ids.size else None, len(ids), 0,
                                                   lengths.ctypes.data if len(ids) else None, *tail, ctypes.byref(aux),
                                                   doc_tok_off.ctypes.data))
        self.n_tokens, self.doc_tok_off = n_tok.value, doc_tok_off
        return call.result(ids, lengths, arrays, doc_tok_off)

    def encode_batch_windows(self, texts_or_buffer, chunk_off=None, doc_chunk_off=None, *, seq_len, stride,
                             score_once=False, out_bits=32, pad_id=0, bos_id=None, eos_id=None, text_ptr=None,
                             n_bytes=None, out_ptr=None, len_ptr=None, cap_rows=None, labels=False, positions=False,
                             segments=False, ignore_label=-100, labels_ptr=None, pos_ptr=None, seg_ptr=None,
                             row_doc=False, row_tok0=False, row_doc_ptr=None, row_tok0_ptr=None):
        """encode_batch_aux for the window layout (mbpe_encoder_encode_batch_windows): the documents of encode_batch,
        the keywords and the result of pack_windows.  The row count depends on the tokens: the host form asks for it
        first, which runs the passes.  The documents' token offsets of the call: self.doc_tok_off."""
        spec = pack_spec(seq_len, "padded", out_bits, pad_id, bos_id, eos_id)
        call = _WinCall(spec, stride, score_once, labels, positions, segments, ignore_label, row_doc, row_tok0)
        head, keep = self._batch_head(texts_or_buffer, chunk_off, doc_chunk_off, text_ptr, n_bytes, spec)
        n_tok = ctypes.c_uint64()
        doc_tok_off = np.zeros(len(keep[-1]), dtype=np.uint64)
        tail = lambda n_rows, aux, win: (ctypes.byref(n_rows), ctypes.byref(n_tok), ctypes.byref(aux),
                                         doc_tok_off.ctypes.data, ctypes.byref(win))
        try:
            out = call.run(lib().mbpe_encoder_encode_batch_windows, head, tail, out_ptr, len_ptr, cap_rows,
                           (labels_ptr, pos_ptr, seg_ptr, row_doc_ptr, row_tok0_ptr))
        finally:
            self.n_rows, self.n_tokens, self.doc_tok_off = getattr(call, "n_rows", None), n_tok.value, doc_tok_off
        return out

    def encode_batch_endmask_windows(self, text_ptr, n_bytes, mask_ptr, singles, doc_off, *, seq_len, stride,
                                     score_once=False, out_bits=32, pad_id=0, bos_id=None, eos_id=None, out_ptr=None,
                                     len_ptr=None, cap_rows=None, labels=False, positions=False, segments=False,
                                     ignore_label=-100, labels_ptr=None, pos_ptr=None, seg_ptr=None, row_doc=False,
                                     row_tok0=False, row_doc_ptr=None, row_tok0_ptr=None):
        """encode_batch_endmask for the window layout (mbpe_encoder_encode_batch_endmask_windows): its text, mask,
        singles and documents, the keywords and the result of pack_windows.  The documents' token offsets:
        self.doc_tok_off."""
        spec = pack_spec(seq_len, "padded", out_bits, pad_id, bos_id, eos_id)
        call = _WinCall(spec, stride, score_once, labels, positions, segments, ignore_label, row_doc, row_tok0)
        sg = _singles(singles)
        docs = np.ascontiguousarray(doc_off, dtype=np.uint64)
        n_tok = ctypes.c_uint64()
        doc_tok_off = np.zeros(len(docs), dtype=np.uint64)
        head = (self._h, _ptr(text_ptr), n_bytes, _ptr(mask_ptr), sg.ctypes.data if len(sg) else None, len(sg),
                docs.ctypes.data, len(docs) - 1, ctypes.byref(spec))
        tail = lambda n_rows, aux, win: (ctypes.byref(n_rows), ctypes.byref(n_tok), ctypes.byref(aux),
                                         doc_tok_off.ctypes.data, ctypes.byref(win))
        try:
            out = call.run(lib().mbpe_encoder_encode_batch_endmask_windows, head, tail, out_ptr, len_ptr, cap_rows,
                           (labels_ptr, pos_ptr, seg_ptr, row_doc_ptr, row_tok0_ptr))
        finally:
            self.n_rows, self.n_tokens, self.doc_tok_off = getattr(call, "n_rows", None), n_tok.value, doc_tok_off
        return out

    def encode_batch_fit(self, texts_or_buffer, chunk_off=None, doc_chunk_off=None, *, seq_len, out_bits=32, pad_id=0,
                         bos_id=None, eos_id=None, text_ptr=None, n_bytes=None, out_ptr=None, len_ptr=None,
                         cap_rows=None, labels=False, positions=False, segments=False, cu_seqlens=False,
                         ignore_label=-100, labels_ptr=None, pos_ptr=None, seg_ptr=None, doc_row=False, doc_col=False,
                         doc_row_ptr=None, doc_col_ptr=None):
        """encode_batch_aux for the fit layout (mbpe_encoder_encode_batch_fit): the documents of encode_batch, the
        keywords and the result of pack_fit.  The plan is made on the host from the documents' token offsets, which
        cross after the passes; the host form asks for the row count first, which runs the passes.  The offsets of
        the call: self.doc_tok_off."""
        spec = _fit_spec(seq_len, out_bits, pad_id, bos_id, eos_id)
        call = _FitCall(spec, labels, positions, segments, cu_seqlens, ignore_label, doc_row, doc_col)
        head, keep = self._batch_head(texts_or_buffer, chunk_off, doc_chunk_off, text_ptr, n_bytes, spec)
        n_tok = ctypes.c_uint64()
        doc_tok_off = np.zeros(len(keep[-1]), dtype=np.uint64)
        tail = lambda n_rows, aux, fit: (ctypes.byref(n_rows), ctypes.byref(n_tok), ctypes.byref(aux),
                                         doc_tok_off.ctypes.data, ctypes.byref(fit))
        try:
            out = call.run(lib().mbpe_encoder_encode_batch_fit, head, tail, len(doc_tok_off) - 1, lambda: doc_tok_off,
                           out_ptr, len_ptr, cap_rows, (labels_ptr, pos_ptr, seg_ptr, doc_row_ptr, doc_col_ptr))
        finally:
            self.n_rows, self.n_tokens, self.doc_tok_off = getattr(call, "n_rows", None), n_tok.value, doc_tok_off
        return out

    def encode_batch_endmask_fit(self, text_ptr, n_bytes, mask_ptr, singles, doc_off, *, seq_len, out_bits=32, pad_id=0,
                                 bos_id=None, eos_id=None, out_ptr=None, len_ptr=None, cap_rows=None, labels=False,
                                 positions=False, segments=False, cu_seqlens=False, ignore_label=-100, labels_ptr=None,
                                 pos_ptr=None, seg_ptr=None, doc_row=False, doc_col=False, doc_row_ptr=None,
                                 doc_col_ptr=None):
        """encode_batch_endmask for the fit layout (mbpe_encoder_encode_batch_endmask_fit): its text, mask, singles
        and documents, the keywords and the result of pack_fit.  The documents' token offsets: self.doc_tok_off."""
        spec = _fit_spec(seq_len, out_bits, pad_id, bos_id, eos_id)
        call = _FitCall(spec, labels, positions, segments, cu_seqlens, ignore_label, doc_row, doc_col)
        sg = _singles(singles)
        docs = np.ascontiguousarray(doc_off, dtype=np.uint64)
        n_tok = ctypes.c_uint64()
        doc_tok_off = np.zeros(len(docs), dtype=np.uint64)
        head = (self._h, _ptr(text_ptr), n_bytes, _ptr(mask_ptr), sg.ctypes.data if len(sg) else None, len(sg),
                docs.ctypes.data, len(docs) - 1, ctypes.byref(spec))
        tail = lambda n_rows, aux, fit: (ctypes.byref(n_rows), ctypes.byref(n_tok), ctypes.byref(aux),
                                         doc_tok_off.ctypes.data, ctypes.byref(fit))
        try:
            out = call.run(lib().mbpe_encoder_encode_batch_endmask_fit, head, tail, len(docs) - 1, lambda: doc_tok_off,
                           out_ptr, len_ptr, cap_rows, (labels_ptr, pos_ptr, seg_ptr, doc_row_ptr, doc_col_ptr))
        finally:
            self.n_rows, self.n_tokens, self.doc_tok_off = getattr(call, "n_rows", None), n_tok.value, doc_tok_off
        return out

    def encode_endmask(self, text_ptr, n_bytes, mask_ptr, singles=None, doc_off=None, dtype=np.uint32, out_ptr=None,
                       cap=None, query=False, byte_off=False, byte_off_ptr=None):
        """n_bytes of text in device memory at text_ptr with its end mask in device memory at mask_ptr, both read in
        place (mbpe_encoder_encode_endmask; what Splitter.split_docs and Splitter.endmask give).  singles: rows
        (start, len, id) of byte ranges that are one token each; doc_off: n_docs + 1 byte offsets at chunk boundaries.
        -> (tokens of dtype uint32 or uint16, doc_tok_off or None); with out_ptr= (device memory for cap tokens; 32
        bits: bit 31 = chunk end) or query=True the token count stands in place of the tokens.
        byte_off=True (host output; mbpe_encoder_encode_endmask_byteoff) appends the n + 1 token byte offsets to the
        result; byte_off_ptr (with out_ptr): device memory for cap + 1 uint64 that receives them."""
        dtype = np.dtype(dtype)
        sg = _singles(singles)
        docs = None if doc_off is None else np.ascontiguousarray(doc_off, dtype=np.uint64)
        n_docs = 0 if docs is None else len(docs) - 1
        tok_off = None if docs is None else np.zeros(n_docs + 1, dtype=np.uint64)
        n, passes = ctypes.c_uint64(), ctypes.c_uint32()
        head = (self._h, _ptr(text_ptr), n_bytes, _ptr(mask_ptr), sg.ctypes.data if len(sg) else None, len(sg),
                None if docs is None else docs.ctypes.data, n_docs)
        mid = (dtype.itemsize * 8, 0 if out_ptr is None else 1)
        tail = (None if tok_off is None else tok_off.ctypes.data, ctypes.byref(n), ctypes.byref(passes))
        if query or out_ptr is not None:
            rc = lib().mbpe_encoder_encode_endmask_byteoff(*head, None if query else _ptr(out_ptr), 0 if query else cap,
                                                           *mid, None if query else _ptr(byte_off_ptr), *tail)
            self.n_out = n.value                     # (reported also where a cap too small is refused)
            _check(rc)
            self.n_passes = passes.value
            return n.value, tok_off
        out = np.zeros(max(n_bytes, 1) if cap is None else max(cap, 1), dtype=dtype)
        boff = np.zeros(len(out) + 1, dtype=np.uint64) if byte_off else None
        rc = lib().mbpe_encoder_encode_endmask_byteoff(*head, out.ctypes.data, n_bytes if cap is None else cap, *mid,
                                                       None if boff is None else boff.ctypes.data, *tail)
        self.n_out = n.value
        _check(rc)
        self.n_passes = passes.value
        if byte_off:
            return out[:n.value].copy(), tok_off, boff[:n.value + 1].copy()
        return out[:n.value].copy(), tok_off

    def encode_batch_endmask(self, text_ptr, n_bytes, mask_ptr, singles, doc_off, *, seq_len, layout="padded",
                             out_bits=32, pad_id=0, bos_id=None, eos_id=None, pad_left=False, trunc_left=False,
                             labels=False, positions=False, segments=False, cu_seqlens=False, ignore_label=-100,
                             out_ptr=None, len_ptr=None, cap_rows=None, labels_ptr=None, pos_ptr=None, seg_ptr=None):
        """encode_endmask and the pack kernel in one call (mbpe_encoder_encode_batch_endmask): the documents doc_off
        describes as one id matrix -> (ids, lengths), or with any of labels / positions / segments / cu_seqlens the
        dict of encode_batch_aux.  The documents' token offsets: self.doc_tok_off.  With out_ptr= (and len_ptr=,
        labels_ptr=, pos_ptr=, seg_ptr=: device memory for cap_rows rows; 0 = a query) the matrices go there and the row
        count is returned; self.n_rows holds it also where a cap_rows too small is refused."""
        spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
        with_aux = labels or positions or segments or cu_seqlens
        call = _AuxCall(spec, labels, positions, segments, cu_seqlens, ignore_label) if with_aux else None
        sg = _singles(singles)
        docs = np.ascontiguousarray(doc_off, dtype=np.uint64)
        n_docs = len(docs) - 1
        n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
        doc_tok_off = np.zeros(n_docs + 1, dtype=np.uint64)
        head = (self._h, _ptr(text_ptr), n_bytes, _ptr(mask_ptr), sg.ctypes.data if len(sg) else None, len(sg),
                docs.ctypes.data, n_docs, ctypes.byref(spec))
        tail = (ctypes.byref(n_rows), ctypes.byref(n_tok))
        fn = lib().mbpe_encoder_encode_batch_endmask
        if out_ptr is not None:
            with_aux = labels_ptr or pos_ptr or seg_ptr
            aux = PackAux(labels_ptr or None, pos_ptr or None, seg_ptr or None, int(ignore_label))
            rc = fn(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail, ctypes.byref(aux) if with_aux else None,
                    doc_tok_off.ctypes.data)
            self.n_rows, self.n_tokens, self.doc_tok_off = n_rows.value, n_tok.value, doc_tok_off
            _check(rc)
            return n_rows.value
        if spec.layout == PACK_PADDED:
            n_rows.value = n_docs                     # known without a query
        else:
            aux = call.device(None, None, None) if call else None
            _check(fn(*head, None, 0, 0, None, *tail, ctypes.byref(aux) if call else None, None))
        ids, lengths = _matrix(n_rows.value, spec)
        aux, arrays = call.host(n_rows.value) if call else (None, None)
        _check(fn(*head, ids.ctypes.data if ids.size else None, len(ids), 0, lengths.ctypes.data if len(ids) else None,
                  *tail, ctypes.byref(aux) if call else None, doc_tok_off.ctypes.data))
        self.n_tokens, self.doc_tok_off = n_tok.value, doc_tok_off
        return call.result(ids, lengths, arrays, doc_tok_off) if call else (ids, lengths)

    def encode_batch_denoise(self, texts_or_buffer, chunk_off=None, doc_chunk_off=None, *, enc_len, dec_len, denoise,
                             out_bits=32, pad_id=0, eos_id=None, decoder_start_id=None, ignore_label=-100, labels=True,
                             row_doc=True, text_ptr=None, n_bytes=None, ptrs=None, cap_rows=None):
        """Encode, span-corrupt and pack twice in one device call (mbpe_encoder_encode_batch_denoise): texts as for
        encode_batch, denoise a DenoiseSpec (denoise_spec()) -> a dict of numpy arrays, one row per unit: "enc_ids"
        [rows, enc_len] and "enc_len" -- the inputs, ending in eos_id --, "dec_ids" [rows, dec_len] and "dec_len" -- the
        targets behind decoder_start_id, ending in eos_id --, "dec_labels" (next-token labels of dec_ids, ignore_label
        elsewhere) and "row_doc" (the row's document).  With ptrs= (a dict of device pointers by those names, e.g.
        torch tensors' data_ptr(), with room for cap_rows rows; an empty dict is a query) the matrices are written
        there and the row count is returned; self.n_rows holds it also where a cap_rows too small is refused.  The
        tokens encoded: self.n_tokens.  Not while set_fim or set_mlm is on."""
        es, ds = _denoise_specs(enc_len, dec_len, out_bits, pad_id, eos_id, decoder_start_id)
        head, keep = self._batch_head(texts_or_buffer, chunk_off, doc_chunk_off, text_ptr, n_bytes, es)
        fn = lib().mbpe_encoder_encode_batch_denoise

        def call(batch, cap, on_dev):
            n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
            rc = fn(*head[:-1], ctypes.byref(denoise), ctypes.byref(es), ctypes.byref(ds), batch, cap, on_dev,
                    ctypes.byref(n_rows), ctypes.byref(n_tok))
            return rc, n_rows.value, n_tok.value
        return self._denoise_done(_denoise_batch(call, len(keep[-1]) - 1, denoise, es, ds, ignore_label, ptrs, cap_rows,
                                                 labels, row_doc))

    def encode_batch_endmask_denoise(self, text_ptr, n_bytes, mask_ptr, singles, doc_off, *, enc_len, dec_len, denoise,
                                     out_bits=32, pad_id=0, eos_id=None, decoder_start_id=None, ignore_label=-100,
                                     labels=True, row_doc=True, ptrs=None, cap_rows=None):
        """encode_batch_denoise for a text and an end mask on the device (mbpe_encoder_encode_batch_endmask_denoise):
        the first five arguments as for encode_batch_endmask, the rest and the result as for encode_batch_denoise."""
        es, ds = _denoise_specs(enc_len, dec_len, out_bits, pad_id, eos_id, decoder_start_id)
        sg = _singles(singles)
        docs = np.ascontiguousarray(doc_off, dtype=np.uint64)
        fn = lib().mbpe_encoder_encode_batch_endmask_denoise

        def call(batch, cap, on_dev):
            n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
            rc = fn(self._h, _ptr(text_ptr), n_bytes, _ptr(mask_ptr), sg.ctypes.data if len(sg) else None, len(sg),
                    docs.ctypes.data, len(docs) - 1, ctypes.byref(denoise), ctypes.byref(es), ctypes.byref(ds), batch, cap,
                    on_dev, ctypes.byref(n_rows), ctypes.byref(n_tok))
            return rc, n_rows.value, n_tok.value
        return self._denoise_done(_denoise_batch(call, len(docs) - 1, denoise, es, ds, ignore_label, ptrs, cap_rows, labels,
                                                 row_doc))

    def _denoise_done(self, res):
        rc, out, n_tok = res
        self.n_tokens = n_tok
        if isinstance(out, int):
            self.n_rows = out
        _check(rc)
        return out

    def _count(self, fn, head, repeat):
        n, passes = ctypes.c_uint64(), ctypes.c_uint32()
        _check(fn(*head, int(repeat), ctypes.byref(n), ctypes.byref(passes)))
        self.n_passes = passes.value
        return n.value

    def count(self, data, chunk_off=None, repeat=1):
        """Encode a host text and count its tokens into the table the encoder keeps (mbpe_encoder_count): what encode
        would return for the same arguments, `repeat` times; no token leaves the device -> the token count (without
        repeat).  counts() reads the table, reset_counts() zeroes it."""
        text = _u8(data)
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        head = (self._h, text.ctypes.data if len(text) else None, len(text), 0,
                None if off is None else off.ctypes.data, 0 if off is None else len(off) - 1)
        return self._count(lib().mbpe_encoder_count, head, repeat)

    def count_device(self, text_ptr, n_bytes, chunk_off, repeat=1):
        """count for n_bytes of text in device memory at text_ptr (read in place)."""
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        head = (self._h, _ptr(text_ptr), n_bytes, 1, None if off is None else off.ctypes.data,
                0 if off is None else len(off) - 1)
        return self._count(lib().mbpe_encoder_count, head, repeat)

    def count_endmask(self, text_ptr, n_bytes, mask_ptr, singles=None, repeat=1):
        """count for a device text with its end mask in device memory (mbpe_encoder_count_endmask; the arguments of
        encode_endmask)."""
        sg = _singles(singles)
        head = (self._h, _ptr(text_ptr), n_bytes, _ptr(mask_ptr), sg.ctypes.data if len(sg) else None, len(sg))
        return self._count(lib().mbpe_encoder_count_endmask, head, repeat)

    def counts(self, out_ptr=None):
        """The table (mbpe_encoder_counts) -> (counts uint64[n_ids], n_other, n_tokens): n_other counts the ids at or
        beyond n_ids, n_tokens is the weighted total, and sum(counts) + n_other == n_tokens.  With out_ptr= (device
        memory for n_ids uint64) the table is written there and n_ids stands in place of the array."""
        n_ids, other, total = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        tail = (ctypes.byref(n_ids), ctypes.byref(other), ctypes.byref(total))
        _check(lib().mbpe_encoder_counts(self._h, None, 0, 0, *tail))
        if out_ptr is not None:
            _check(lib().mbpe_encoder_counts(self._h, _ptr(out_ptr), n_ids.value, 1, *tail))
            return n_ids.value, other.value, total.value
        out = np.zeros(n_ids.value, dtype=np.uint64)
        _check(lib().mbpe_encoder_counts(self._h, out.ctypes.data, len(out), 0, *tail))
        return out, other.value, total.value

    def reset_counts(self):
        """Zero the table (mbpe_encoder_counts_reset)."""
        _check(lib().mbpe_encoder_counts_reset(self._h))

    def pack_ms(self):
        """Device time of the pack kernel of the latest encode_batch (mbpe_encoder_pack_ms)."""
        ms = ctypes.c_float()
        _check(lib().mbpe_encoder_pack_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def kernel_ms(self):
        """Device time of the latest call (mbpe_encoder_kernel_ms)."""
        ms = ctypes.c_float()
        _check(lib().mbpe_encoder_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def pass_tokens(self):
        """Tokens that entered every pass of the latest call (mbpe_encoder_pass_tokens) -> list."""
        n = ctypes.c_uint32()
        _check(lib().mbpe_encoder_pass_tokens(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint64)
        _check(lib().mbpe_encoder_pass_tokens(self._h, out.ctypes.data, n.value, ctypes.byref(n)))
        return [int(v) for v in out[:n.value]]

    def alloc_count(self):
        """Device allocations made so far (mbpe_encoder_alloc_count)."""
        n = ctypes.c_uint64()
        _check(lib().mbpe_encoder_alloc_count(self._h, ctypes.byref(n)))
        return n.value

    def dedup_stats(self):
        """The latest call on the "dedup" route (mbpe_encoder_dedup_stats) -> dict: n_chunks (those the deduper kept),
        n_unique, n_unique_bytes, n_unique_tokens, expand_ms.  MbpeError(ERR_STATE) when that call did not dedup."""
        v = [ctypes.c_uint64() for _ in range(4)]
        ms = ctypes.c_float()
        _check(lib().mbpe_encoder_dedup_stats(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(ms)))
        names = ("n_chunks", "n_unique", "n_unique_bytes", "n_unique_tokens")
        return dict(zip(names, (x.value for x in v)), expand_ms=ms.value)


class Decoder:
    """One mbpe_decoder: Tokenizer::decode (Tokenizer.h:725-751) on a HIP device.  specials: {id: bytes}."""

    def __init__(self, merges, specials=None, device=0):
        self._h = ctypes.c_void_p()
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
        items = list((specials or {}).items())
        ids = np.array([k for k, _ in items], dtype=np.uint32)
        blob = b"".join(bytes(v) for _, v in items)
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(v) for _, v in items], dtype=np.uint64) if items else []
        b = np.frombuffer(blob, dtype=np.uint8)
        _check(lib().mbpe_decoder_create(device, m.ctypes.data if len(m) else None, len(m),
                                         ids.ctypes.data if len(ids) else None, b.ctypes.data if len(b) else None,
                                         off.ctypes.data if len(ids) else None, len(ids), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().mbpe_decoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def decode(self, tokens, with_invalid=False):
        """Host tokens -> bytes (mbpe_decode_tokens: a size query, then the decode)."""
        t = np.ascontiguousarray(tokens, dtype=np.uint32)
        tp = t.ctypes.data if len(t) else None
        n, bad = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mbpe_decode_tokens(self._h, tp, len(t), 0, None, 0, 0, ctypes.byref(n), ctypes.byref(bad)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_decode_tokens(self._h, tp, len(t), 0, out.ctypes.data, n.value, 0, ctypes.byref(n),
                                        ctypes.byref(bad)))
        data = out[:n.value].tobytes()
        return (data, bad.value) if with_invalid else data

    def decode_device(self, ptr, n_tokens, out_ptr, cap):
        """n_tokens uint32 ids in device memory at ptr -> bytes in device memory at out_ptr (0: size query; room for
        cap bytes) -> (decoded length, ids that decoded to nothing)."""
        n, bad = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mbpe_decode_tokens(self._h, ctypes.c_void_p(ptr) if ptr else None, n_tokens, 1,
                                        ctypes.c_void_p(out_ptr) if out_ptr else None, cap, 1,
                                        ctypes.byref(n), ctypes.byref(bad)))
        return n.value, bad.value

    def decode_batch(self, docs, with_invalid=False, dtype=np.uint32):
        """A list of token arrays -> the list of their texts, in one device call each for the lengths and the bytes
        (mbpe_decode_batch).  dtype uint16 sends the ids as plain 16-bit ids."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint32), np.dtype(np.uint16)):
            raise ValueError("dtype must be uint32 or uint16")
        parts = [np.ascontiguousarray(t, dtype=dtype).reshape(-1) for t in docs]
        tok_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            tok_off[1:] = np.cumsum([len(t) for t in parts], dtype=np.uint64)
        t = np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)
        tp = t.ctypes.data if len(t) else None
        byte_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        n, bad = ctypes.c_uint64(), ctypes.c_uint64()
        args = (self._h, tp, len(t), dtype.itemsize * 8, 0, tok_off.ctypes.data, len(parts))
        _check(lib().mbpe_decode_batch(*args, None, 0, 0, byte_off.ctypes.data, ctypes.byref(n), ctypes.byref(bad)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_decode_batch(*args, out.ctypes.data, n.value, 0, byte_off.ctypes.data, ctypes.byref(n),
                                       ctypes.byref(bad)))
        data = out[:n.value].tobytes()
        texts = [data[int(a):int(b)] for a, b in zip(byte_off[:-1], byte_off[1:])]
        return (texts, bad.value) if with_invalid else texts

    def decode_batch_device(self, ptr, n_tokens, doc_tok_off, out_ptr, cap, token_bits=32):
        """n_tokens ids of token_bits bits in device memory at ptr, document i being tokens doc_tok_off[i] ..
        doc_tok_off[i + 1] -> bytes in device memory at out_ptr (0: query; room for cap bytes) -> (doc_byte_off,
        decoded length, ids that decoded to nothing): document i's text is bytes doc_byte_off[i] .. doc_byte_off[i + 1]."""
        tok_off = np.ascontiguousarray(doc_tok_off, dtype=np.uint64)
        byte_off = np.zeros(len(tok_off), dtype=np.uint64)
        n, bad = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mbpe_decode_batch(self._h, ctypes.c_void_p(ptr) if ptr else None, n_tokens, token_bits, 1,
                                       tok_off.ctypes.data if len(tok_off) else None, max(len(tok_off), 1) - 1,
                                       ctypes.c_void_p(out_ptr) if out_ptr else None, cap, 1,
                                       byte_off.ctypes.data, ctypes.byref(n), ctypes.byref(bad)))
        return byte_off, n.value, bad.value

    def decode_slots_device(self, ptr, n_slots, slot_bits, end_bit, barrier, out_ptr, cap):
        """The same for device-resident slots in a layout of Trainer.stream_device() (mbpe_decode_slots)."""
        n, bad = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mbpe_decode_slots(self._h, ctypes.c_void_p(ptr) if ptr else None, n_slots, slot_bits, end_bit,
                                       0xFFFFFFFF if barrier is None else barrier,
                                       ctypes.c_void_p(out_ptr) if out_ptr else None, cap, 1,
                                       ctypes.byref(n), ctypes.byref(bad)))
        return n.value, bad.value

    def kernel_ms(self):
        """Device time of the latest call (mbpe_decoder_kernel_ms)."""
        ms = ctypes.c_float()
        _check(lib().mbpe_decoder_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def alloc_count(self):
        """Device allocations made so far (mbpe_decoder_alloc_count)."""
        n = ctypes.c_uint64()
        _check(lib().mbpe_decoder_alloc_count(self._h, ctypes.byref(n)))
        return n.value


class Splitter:
    """One mbpe_splitter: the gpt2 / gpt4 pre-split on the device (pattern = split_pattern("gpt2") or ("gpt4"))."""

    def __init__(self, pattern, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().mbpe_splitter_create(device, pattern.encode("utf-8"), ctypes.byref(self._h)))
        self._keep = None

    def close(self):
        if self._h:
            lib().mbpe_splitter_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        _check(lib().mbpe_splitter_set_option(self._h, name.encode(), int(value)))

    def split(self, data=None, offsets=True, mask_ptr=None, text_ptr=None, n_bytes=None, cap_chunks=None):
        """Splits data (host bytes), or n_bytes of device memory at text_ptr.  Returns the number of chunks, or with
        offsets the uint64 offsets [n_chunks + 1] that presplit gives.  mask_ptr: device memory for the end mask
        (mask_bytes(n) of it); otherwise the mask stays in the splitter, see endmask().  cap_chunks: the capacity
        handed to the library with the offsets array (default: n_bytes, which always suffices)."""
        if text_ptr is None:
            text = _u8(data)
            self._keep = text
            ptr, n, on_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            ptr, n, on_dev = ctypes.c_void_p(text_ptr), n_bytes, 1
        count = ctypes.c_uint64()
        mask = None if mask_ptr is None else ctypes.c_void_p(mask_ptr)
        if not offsets:
            _check(lib().mbpe_splitter_split(self._h, ptr, n, on_dev, mask, None, 0, ctypes.byref(count)))
            return count.value
        if cap_chunks is None:
            cap_chunks = n          # always enough: no chunk is empty
        off = np.zeros(cap_chunks + 1, dtype=np.uint64)
        _check(lib().mbpe_splitter_split(self._h, ptr, n, on_dev, mask, off.ctypes.data, cap_chunks, ctypes.byref(count)))
        return off[:count.value + 1]

    def split_docs(self, data=None, doc_off=None, names=(), mask_ptr=None, text_ptr=None, n_bytes=None, cap_ranges=None):
        """Splits the documents data[doc_off[i]:doc_off[i + 1]] (host bytes, or n_bytes of device memory at text_ptr)
        each on its own, around the occurrences of names (a list of bytes) and around NUL-led parts
        (mbpe_splitter_split_docs) -> (number of chunks, ranges as int64 [n_ranges, 3] rows (start, len, name index or
        SPLIT_RAW)).  The mask goes to mask_ptr (device memory) or stays in the splitter, see endmask().  cap_ranges:
        the capacity handed to the library for the ranges (default: they are read from the splitter)."""
        if text_ptr is None:
            text = _u8(data)
            self._keep = text
            ptr, n, on_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            ptr, n, on_dev = ctypes.c_void_p(text_ptr), n_bytes, 1
        docs = np.ascontiguousarray(doc_off, dtype=np.uint64)
        names = [bytes(x) for x in names]
        name_off = np.zeros(len(names) + 1, dtype=np.uint64)
        if names:
            name_off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        count, n_ranges = ctypes.c_uint64(), ctypes.c_uint64()
        mask = None if mask_ptr is None else ctypes.c_void_p(mask_ptr)
        rows = np.zeros(0 if cap_ranges is None else max(cap_ranges, 1), dtype=SINGLE)
        rc = lib().mbpe_splitter_split_docs(self._h, ptr, n, on_dev, docs.ctypes.data, len(docs) - 1, blob.ctypes.data,
                                            name_off.ctypes.data, len(names), mask,
                                            None if cap_ranges is None else rows.ctypes.data, cap_ranges or 0,
                                            ctypes.byref(n_ranges), ctypes.byref(count))
        self.n_ranges = n_ranges.value
        _check(rc)
        if cap_ranges is None:
            p, k = ctypes.c_void_p(), ctypes.c_uint64()
            _check(lib().mbpe_splitter_ranges(self._h, ctypes.byref(p), ctypes.byref(k)))
            rows = np.zeros(k.value, dtype=SINGLE)
            if k.value:
                ctypes.memmove(rows.ctypes.data, p, k.value * SINGLE.itemsize)
        rows = rows[:n_ranges.value]
        out = np.stack([rows["start"].astype(np.int64), rows["len"].astype(np.int64), rows["id"].astype(np.int64)],
                       axis=1) if len(rows) else np.zeros((0, 3), dtype=np.int64)
        return count.value, out

    def find_ms(self):
        """Device time of the latest split_docs call's search for the names (mbpe_splitter_find_ms)."""
        ms = ctypes.c_float()
        _check(lib().mbpe_splitter_find_ms(self._h, ctypes.byref(ms)))
        return ms.value

    @staticmethod
    def mask_bytes(n_bytes):
        return (n_bytes + 15) // 16 * 2 + 16

    def endmask(self):
        """(device address of the latest call's end mask, its size in bytes, device address of that call's text);
        all owned by the splitter (or, the text, by the caller) and valid until its next call."""
        m, nb, t = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
        _check(lib().mbpe_splitter_endmask(self._h, ctypes.byref(m), ctypes.byref(nb), ctypes.byref(t)))
        return m.value, nb.value, t.value

    def kernel_ms(self):
        ms = ctypes.c_float()
        _check(lib().mbpe_splitter_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def alloc_count(self):
        n = ctypes.c_uint64()
        _check(lib().mbpe_splitter_alloc_count(self._h, ctypes.byref(n)))
        return n.value

    def host_spans(self):
        """(host spans, text bytes in them) of the latest call."""
        n, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mbpe_splitter_host_spans(self._h, ctypes.byref(n), ctypes.byref(b)))
        return n.value, b.value


class Deduper:
    """One mbpe_dedup: the distinct chunks of a chunked text in order of first occurrence, with their counts."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().mbpe_dedup_create(device, ctypes.byref(self._h)))
        self._keep = None
        self.n_unique = self.n_unique_bytes = 0

    def close(self):
        if self._h:
            lib().mbpe_dedup_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        _check(lib().mbpe_dedup_set_option(self._h, name.encode(), int(value)))

    def _done(self, rc, nu, nb):
        self.n_unique, self.n_unique_bytes = nu.value, nb.value
        _check(rc)
        return nu.value, nb.value

    def chunks(self, data, chunk_off, text_ptr=None, n_bytes=None):
        """The chunks data[chunk_off[c]:chunk_off[c + 1]] (host bytes, or n_bytes of device memory at text_ptr) ->
        (n_unique, n_unique_bytes).  Empty chunks vanish."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        if text_ptr is None:
            text = _u8(data)
            ptr, n, on_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            text, ptr, n, on_dev = None, ctypes.c_void_p(text_ptr), n_bytes, 1
        self._keep = (text, off)
        nu, nb = ctypes.c_uint64(), ctypes.c_uint64()
        return self._done(lib().mbpe_dedup_chunks(self._h, ptr, n, on_dev, off.ctypes.data, len(off) - 1, ctypes.byref(nu),
                                                  ctypes.byref(nb)), nu, nb)

    def chunks_endmask(self, text_ptr, n_bytes, mask_ptr):
        """n_bytes of device text at text_ptr with the end mask at mask_ptr (Splitter.endmask), both read in place ->
        (n_unique, n_unique_bytes)."""
        nu, nb = ctypes.c_uint64(), ctypes.c_uint64()
        return self._done(lib().mbpe_dedup_chunks_endmask(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, n_bytes,
                                                          ctypes.c_void_p(mask_ptr) if mask_ptr else None,
                                                          ctypes.byref(nu), ctypes.byref(nb)), nu, nb)

    def result(self):
        """Device addresses (text, end mask, weights u32, first_chunk u64) of the latest result, owned by the deduper
        and valid until its next call."""
        t, m, w, f = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().mbpe_dedup_result(self._h, ctypes.byref(t), ctypes.byref(m), ctypes.byref(w), ctypes.byref(f)))
        return t.value, m.value, w.value, f.value

    def get(self, cap_bytes=None, cap_chunks=None):
        """Host copies of the latest result -> (text bytes, chunk_off uint64 [n_unique + 1], weights uint32,
        first_chunk uint64).  cap_bytes / cap_chunks: the capacities handed to the library (default: the result's
        sizes)."""
        nb = self.n_unique_bytes if cap_bytes is None else cap_bytes
        nu = self.n_unique if cap_chunks is None else cap_chunks
        text = np.zeros(max(nb, 1), dtype=np.uint8)
        off = np.zeros(nu + 1, dtype=np.uint64)
        w = np.zeros(max(nu, 1), dtype=np.uint32)
        f = np.zeros(max(nu, 1), dtype=np.uint64)
        _check(lib().mbpe_dedup_get(self._h, text.ctypes.data, off.ctypes.data, w.ctypes.data, f.ctypes.data, nb, nu))
        return (text[:self.n_unique_bytes].tobytes(), off[:self.n_unique + 1], w[:self.n_unique], f[:self.n_unique])

    def unique_of(self):
        """Host copy of the inverse map of the latest result (option "map"; mbpe_dedup_get_map) -> uint32 array with one
        entry per chunk the deduper kept: the index of the unique chunk that has its bytes."""
        n = ctypes.c_uint64()
        _check(lib().mbpe_dedup_get_map(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(lib().mbpe_dedup_get_map(self._h, out.ctypes.data, n.value, ctypes.byref(n)))
        return out[:n.value]

    def map_device(self):
        """Device address of unique_of (u32) and the number of chunks kept (mbpe_dedup_map), valid until the next call."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _check(lib().mbpe_dedup_map(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def kernel_ms(self):
        ms = ctypes.c_float()
        _check(lib().mbpe_dedup_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def alloc_count(self):
        n = ctypes.c_uint64()
        _check(lib().mbpe_dedup_alloc_count(self._h, ctypes.byref(n)))
        return n.value


class WordCount:
    """One mbpe_wordcount: the distinct chunks of a corpus that is added piece by piece, in order of first occurrence
    over all pieces, with their counts -- one dedup of the pieces' chunk lists laid end to end."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().mbpe_wordcount_create(device, ctypes.byref(self._h)))
        self._keep = None
        self.n_unique = self.n_unique_bytes = 0

    def close(self):
        if self._h:
            lib().mbpe_wordcount_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        """"max_chunk_bytes", "hash_bits": the owned deduper's; MbpeError(ERR_STATE) once a piece has been added."""
        _check(lib().mbpe_wordcount_set_option(self._h, name.encode(), int(value)))

    def _done(self, rc, nu, nb):
        _check(rc)
        self.n_unique, self.n_unique_bytes = nu.value, nb.value
        return nu.value, nb.value

    def add(self, data, chunk_off, repeat=1, text_ptr=None, n_bytes=None):
        """One piece: the chunks data[chunk_off[c]:chunk_off[c + 1]] (host bytes, or n_bytes of device memory at
        text_ptr), counted `repeat` times -> the table's (n_unique, n_unique_bytes) after it."""
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        if text_ptr is None:
            text = _u8(data)
            ptr, n, on_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            text, ptr, n, on_dev = None, ctypes.c_void_p(text_ptr), n_bytes, 1
        self._keep = (text, off)
        nu, nb = ctypes.c_uint64(), ctypes.c_uint64()
        return self._done(lib().mbpe_wordcount_add(self._h, ptr, n, on_dev, off.ctypes.data, len(off) - 1, repeat,
                                                   ctypes.byref(nu), ctypes.byref(nb)), nu, nb)

    def add_endmask(self, text_ptr, n_bytes, mask_ptr, repeat=1):
        """One piece: n_bytes of device text at text_ptr with the end mask at mask_ptr (Splitter.endmask), both read in
        place, counted `repeat` times -> the table's (n_unique, n_unique_bytes) after it."""
        nu, nb = ctypes.c_uint64(), ctypes.c_uint64()
        return self._done(lib().mbpe_wordcount_add_endmask(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, n_bytes,
                                                           ctypes.c_void_p(mask_ptr) if mask_ptr else None, repeat,
                                                           ctypes.byref(nu), ctypes.byref(nb)), nu, nb)

    def result(self):
        """Device addresses (text, end mask, weights u32, first_chunk u64) of the table, owned by the object and valid
        until its next add or reset: Trainer.load_corpus_endmask_weighted takes them as they are."""
        t, m, w, f = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().mbpe_wordcount_result(self._h, ctypes.byref(t), ctypes.byref(m), ctypes.byref(w), ctypes.byref(f)))
        return t.value, m.value, w.value, f.value

    def get(self):
        """Host copies of the table -> (text bytes, chunk_off uint64 [n_unique + 1], weights uint32, first_chunk uint64)."""
        nb, nu = self.n_unique_bytes, self.n_unique
        text = np.zeros(max(nb, 1), dtype=np.uint8)
        off = np.zeros(nu + 1, dtype=np.uint64)
        w = np.zeros(max(nu, 1), dtype=np.uint32)
        f = np.zeros(max(nu, 1), dtype=np.uint64)
        _check(lib().mbpe_wordcount_get(self._h, text.ctypes.data, off.ctypes.data, w.ctypes.data, f.ctypes.data, nb, nu))
        return text[:nb].tobytes(), off, w[:nu], f[:nu]

    def stats(self):
        """-> dict: n_pieces, n_chunks_total (repeats included), n_unique, n_unique_bytes."""
        v = [ctypes.c_uint64() for _ in range(4)]
        _check(lib().mbpe_wordcount_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("n_pieces", "n_chunks_total", "n_unique", "n_unique_bytes"), (x.value for x in v)))

    def reset(self):
        """Empty again; the device buffers are kept."""
        _check(lib().mbpe_wordcount_reset(self._h))
        self.n_unique = self.n_unique_bytes = 0

    def export(self):
        """The table as bytes (mbpe_wordcount_export): header, ends, weights, first_chunk, text.  The object is
        unchanged and goes on counting, so this is also a checkpoint.  MbpeError(ERR_OVERFLOW) once a count has
        reached 2^31."""
        n = ctypes.c_uint64()
        _check(lib().mbpe_wordcount_export_size(self._h, ctypes.byref(n)))
        blob = np.zeros(n.value, dtype=np.uint8)
        _check(lib().mbpe_wordcount_export(self._h, blob.ctypes.data, n.value, ctypes.byref(n)))
        return blob[:n.value].tobytes()

    def merge(self, other):
        """Another table -- the bytes of export(), from any process or device, or a WordCount on the same device, which
        stays unchanged -- folded into this one: afterwards this is the count of its own pieces followed by the
        other's, bit for bit what adding all of them here gives.  Merge in piece order for the `first` tie-break's
        order; any order gives the same weights.  A blob is checked before anything changes: MbpeError(ERR_ARG) naming
        the rule, the table as it was.  -> the table's (n_unique, n_unique_bytes) after it."""
        if isinstance(other, WordCount):
            _check(lib().mbpe_wordcount_merge(self._h, other._h))
            st = self.stats()
            self.n_unique, self.n_unique_bytes = st["n_unique"], st["n_unique_bytes"]
            return self.n_unique, self.n_unique_bytes
        blob = _u8(other)
        nu, nb = ctypes.c_uint64(), ctypes.c_uint64()
        return self._done(lib().mbpe_wordcount_merge_blob(self._h, blob.ctypes.data, len(blob), ctypes.byref(nu),
                                                          ctypes.byref(nb)), nu, nb)

    def kernel_ms(self):
        """Device time of the latest add or merge: the deduper's kernels (add) and the fold's, with the check of a blob."""
        ms = ctypes.c_float()
        _check(lib().mbpe_wordcount_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def alloc_count(self):
        n = ctypes.c_uint64()
        _check(lib().mbpe_wordcount_alloc_count(self._h, ctypes.byref(n)))
        return n.value


class Trainer:
    """One mbpe_ctx.  Mirrors the order of Tokenizer::train (Tokenizer.h:489-598)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().mbpe_create(device, ctypes.byref(self._h)))
        self._keep = None
        self.vocab_size = 0

    def close(self):
        if self._h:
            lib().mbpe_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        _check(lib().mbpe_set_option(self._h, name.encode(), int(value)))

    def load_corpus(self, data, chunk_off=None):
        text = _u8(data)
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        self._keep = (text, off)
        _check(lib().mbpe_load_corpus(self._h, text.ctypes.data if len(text) else None, len(text),
                                      None if off is None else off.ctypes.data,
                                      0 if off is None else len(off) - 1, 0))

    def load_corpus_ranges(self, data, starts, ends):
        text = _u8(data)
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        en = np.ascontiguousarray(ends, dtype=np.uint64)
        self._keep = (text, st, en)
        _check(lib().mbpe_load_corpus_ranges(self._h, text.ctypes.data if len(text) else None, len(text),
                                             st.ctypes.data if len(st) else None, en.ctypes.data if len(en) else None,
                                             len(st), 0))

    def load_corpus_device(self, dev_ptr, n_bytes, chunk_off=None, keep=None):
        """dev_ptr: device address of n_bytes corpus bytes (e.g. torch tensor .data_ptr())."""
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        self._keep = (keep, off)
        _check(lib().mbpe_load_corpus(self._h, ctypes.c_void_p(dev_ptr), n_bytes,
                                      None if off is None else off.ctypes.data,
                                      0 if off is None else len(off) - 1, 1))

    def load_corpus_endmask(self, mask_ptr, data=None, text_ptr=None, n_bytes=None, keep=None):
        """A chunked corpus whose end mask is in device memory at mask_ptr (Splitter.split / Splitter.endmask); the
        text is host bytes (data) or n_bytes of device memory at text_ptr, taken in place."""
        if text_ptr is None:
            text = _u8(data)
            self._keep = (text, keep)
            _check(lib().mbpe_load_corpus_endmask(self._h, text.ctypes.data if len(text) else None, len(text), 0,
                                                  ctypes.c_void_p(mask_ptr)))
        else:
            self._keep = (keep,)
            _check(lib().mbpe_load_corpus_endmask(self._h, ctypes.c_void_p(text_ptr), n_bytes, 1,
                                                  ctypes.c_void_p(mask_ptr)))

    def load_corpus_weighted(self, data, chunk_off, weights):
        """Chunk c stands for weights[c] occurrences (mbpe_load_corpus_weighted): the training then runs on 32-bit
        tokens and counts what the expanded corpus holds."""
        text = _u8(data)
        off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        w = np.ascontiguousarray(weights, dtype=np.uint32)
        if len(w) != len(off) - 1:
            raise ValueError("one weight per chunk")
        self._keep = (text, off, w)
        _check(lib().mbpe_load_corpus_weighted(self._h, text.ctypes.data if len(text) else None, len(text),
                                               off.ctypes.data, len(off) - 1, 0, w.ctypes.data if len(w) else None))

    def load_corpus_endmask_weighted(self, mask_ptr, weights=None, data=None, text_ptr=None, n_bytes=None,
                                     weights_ptr=None, n_weights=None, keep=None):
        """load_corpus_endmask with one weight per end bit of the mask: weights (host array) or n_weights u32 of device
        memory at weights_ptr -- Deduper.result() goes in as it is."""
        if weights_ptr is None:
            w = np.ascontiguousarray(weights, dtype=np.uint32)
            wp, nw, w_dev = (w.ctypes.data if len(w) else None), len(w), 0
        else:
            w, wp, nw, w_dev = None, ctypes.c_void_p(weights_ptr), n_weights, 1
        if text_ptr is None:
            text = _u8(data)
            tp, n, t_dev = (text.ctypes.data if len(text) else None), len(text), 0
        else:
            text, tp, n, t_dev = None, ctypes.c_void_p(text_ptr), n_bytes, 1
        self._keep = (text, w, keep)
        _check(lib().mbpe_load_corpus_endmask_weighted(self._h, tp, n, t_dev, ctypes.c_void_p(mask_ptr), wp, nw, w_dev))

    def pair_count_u8(self, want_table=True):
        table = np.zeros(65536, dtype=np.uint32) if want_table else None
        _check(lib().mbpe_pair_count_u8(self._h, None if table is None else table.ctypes.data))
        return table

    def train_begin(self, vocab_size, prior_merges=None):
        """Returns NEED_EXCHANGE in external-transport mode, else OK.  prior_merges ([n, 2]): continue from these
        merges instead of from raw bytes (mbpe_train_begin_from).  Beyond the 16-bit slot format that is MbpeError(ERR_VOCAB)
        unless set_option("resume_wide", 1) was called: then the training continues on 32-bit tokens, from the slot
        stream's handover or, when the prior merges already reach it, directly (vocabularies up to 2^24, one rank;
        `first` also needs "first_wide")."""
        if prior_merges is None:
            rc = _check(lib().mbpe_train_begin(self._h, vocab_size))
        else:
            m = _merges(prior_merges)
            rc = _check(lib().mbpe_train_begin_from(self._h, vocab_size, m.ctypes.data if len(m) else None, len(m)))
        self.vocab_size = vocab_size
        return rc

    def train_steps(self, n_steps):
        """Returns the number of merges made (external-transport mode: NEED_EXCHANGE / OK code)."""
        done = ctypes.c_uint32()
        rc = _check(lib().mbpe_train_steps(self._h, n_steps, ctypes.byref(done)))
        return rc if self._external else done.value

    def train_sequences(self, n_sequences):
        """Runs up to n_sequences batch sequences (see mbpe_train_sequences); returns the merges they committed."""
        done = ctypes.c_uint32()
        _check(lib().mbpe_train_sequences(self._h, n_sequences, ctypes.byref(done)))
        return done.value

    _external = False

    def comm_init_external(self, rank, n_ranks):
        _check(lib().mbpe_comm_init_external(self._h, rank, n_ranks))
        self._external = n_ranks > 1

    def exchange_buffer(self):
        """(device pointer, number of u32) of the buffer to sum-all-reduce across ranks."""
        p = ctypes.c_void_p()
        n = ctypes.c_uint64()
        _check(lib().mbpe_comm_exchange_buffer(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def exchange_done(self):
        return _check(lib().mbpe_comm_exchange_done(self._h))

    def train_result(self):
        cap = max(self.vocab_size - 256, 1)
        merges = np.zeros((cap, 2), dtype=np.uint32)
        counts = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_uint32()
        _check(lib().mbpe_train_result(self._h, merges.ctypes.data, counts.ctypes.data, cap, ctypes.byref(n)))
        return merges[:n.value].copy(), counts[:n.value].copy()

    def train_lexical(self, data, vocab_size, chunk_off=None):
        return self.train(data, vocab_size, chunk_off, conflict_resolution=1)

    def train(self, data, vocab_size, chunk_off=None, conflict_resolution=1, prior_merges=None, weights=None):
        """conflict_resolution: 1 = lexical, 0 = first (mbpe_train).  prior_merges: continue from them (mbpe_train_from);
        the result then starts with them, with counts of -1.  Options are taken from the context: "resume_wide" 1 lets a
        continuation pass the 16-bit slot format (see train_begin).  weights: one per chunk (load_corpus_weighted); the
        training then runs on 32-bit tokens, and the context's "conflict_resolution" is left as this call set it."""
        if weights is not None:
            self.load_corpus_weighted(data, chunk_off, weights)
            self.set_option("conflict_resolution", conflict_resolution)
            self.train_begin(vocab_size, prior_merges if prior_merges is not None and len(prior_merges) else None)
            self.train_steps(vocab_size - 256)
            merges, counts = self.train_result()
            return merges, counts, self.stats()
        text = _u8(data)
        prior = _merges(prior_merges)
        off = None if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.uint64)
        cap = max(vocab_size - 256, 1)
        merges = np.zeros((cap, 2), dtype=np.uint32)
        counts = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_uint32()
        st = Stats()
        _check(lib().mbpe_train_from(self._h, text.ctypes.data if len(text) else None, len(text),
                                     None if off is None else off.ctypes.data,
                                     0 if off is None else len(off) - 1, vocab_size, conflict_resolution,
                                     prior.ctypes.data if len(prior) else None, len(prior),
                                     merges.ctypes.data, counts.ctypes.data, ctypes.byref(n),
                                     ctypes.byref(st)))
        self.vocab_size = vocab_size
        return merges[:n.value].copy(), counts[:n.value].copy(), st.as_dict()

    def stats(self):
        st = Stats()
        _check(lib().mbpe_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def stream(self):
        n = ctypes.c_uint64()
        _check(lib().mbpe_get_stream(self._h, None, None, 0, ctypes.byref(n)))
        toks = np.zeros(max(n.value, 1), dtype=np.uint32)
        ends = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_get_stream(self._h, toks.ctypes.data, ends.ctypes.data, n.value, ctypes.byref(n)))
        return toks[:n.value], ends[:n.value]

    def stream_device(self):
        """(device pointer, n_slots, slot_bits, end_bit, barrier or None) of the live slot stream (see
        mbpe_stream_device)."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        bits, end, bar = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().mbpe_stream_device(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(bits), ctypes.byref(end),
                                        ctypes.byref(bar)))
        return p.value, n.value, bits.value, end.value, (None if bar.value == 0xFFFFFFFF else bar.value)

    def decode_stream(self):
        """The live stream expanded with the merges made so far (mbpe_decode_stream) -> bytes."""
        n = ctypes.c_uint64()
        _check(lib().mbpe_decode_stream(self._h, None, 0, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_decode_stream(self._h, out.ctypes.data, n.value, 0, ctypes.byref(n)))
        return out[:n.value].tobytes()

    def decode_stream_device(self, out_ptr, cap):
        """The same into device memory at out_ptr (0: size query; room for cap bytes) -> decoded length."""
        n = ctypes.c_uint64()
        _check(lib().mbpe_decode_stream(self._h, ctypes.c_void_p(out_ptr) if out_ptr else None, cap, 1, ctypes.byref(n)))
        return n.value

    def table_device(self):
        """(device pointer, vshift) of the dense pair table (see mbpe_table_device)."""
        p, v = ctypes.c_void_p(), ctypes.c_uint32()
        _check(lib().mbpe_table_device(self._h, ctypes.byref(p), ctypes.byref(v)))
        return p.value, v.value

    def pairs(self):
        n = ctypes.c_uint64()
        _check(lib().mbpe_get_pairs(self._h, None, None, None, 0, ctypes.byref(n)))
        a = np.zeros(max(n.value, 1), dtype=np.uint32)
        b = np.zeros(max(n.value, 1), dtype=np.uint32)
        c = np.zeros(max(n.value, 1), dtype=np.int32)
        _check(lib().mbpe_get_pairs(self._h, a.ctypes.data, b.ctypes.data, c.ctypes.data, n.value, ctypes.byref(n)))
        return a[:n.value], b[:n.value], c[:n.value]

    def pairs_dict(self):
        a, b, c = self.pairs()
        return {(int(x), int(y)): int(z) for x, y, z in zip(a, b, c)}

    def compact(self):
        _check(lib().mbpe_compact(self._h))

    def comm_init(self, uid, rank, n_ranks):
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
        _check(lib().mbpe_comm_init(self._h, buf, rank, n_ranks))


def comm_unique_id():
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(lib().mbpe_comm_unique_id(buf))
    return bytes(buf)


class Tokenizer:
    """Binding of include/mbpe_tokenizer.h: the host-side mirror of the reference Tokenizer."""

    FIRST, LEXICAL = 0, 1

    def __init__(self, pattern=""):
        self._h = ctypes.c_void_p()
        _check(lib().mbpe_tok_create(pattern.encode("utf-8"), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().mbpe_tok_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_special_tokens_from_file(self, text):
        b = text if isinstance(text, bytes) else text.encode("utf-8")
        _check(lib().mbpe_tok_set_special_tokens(self._h, b, len(b)))

    def train(self, data, vocab_size, conflict_resolution=1, verbose=False, device=0, device_split=False,
              resume=False, dedup=False, min_frequency=0, max_token_length=0):
        """min_frequency, max_token_length (here, in train_from_iterator and train_files; mbpe_tok_set_train_limits):
        the stopping rules.  The training ends when the best pair left occurs fewer than min_frequency times, and no
        new token is longer than max_token_length bytes (at least 2; the merges a resumed training starts from stay):
        pairs that would make one are never chosen, and the training ends when no other pair is left.  0: off.  The
        tokenizer then holds fewer merges than vocab_size asks for.  With either the training makes one pass per
        merge over the corpus it is given: combine with dedup=True, so that a pass runs over the distinct chunks.
        dedup: split as asked, deduplicate the chunks on the device and train on the distinct ones with their
        counts (mbpe_tok_set_train_dedup): same merges, counts, .model and .vocab.  Meant for the `first` tie-break,
        for vocabularies beyond the 16-bit slot format and with resume; the lexical tie-break within the slot format
        is faster without it.  A tokenizer without a pattern has one chunk and trains slowly this way.
        resume: continue from the merges the tokenizer holds (loaded, set or trained) up to vocab_size instead of
        starting from raw bytes (mbpe_tok_train_continue); pattern and special tokens stay.  Vocabularies up to 2^24,
        either tie-break: beyond the 16-bit slot format the continuation runs on 32-bit tokens ("resume_wide").
        device_split: the gpt2 / gpt4 pre-split runs on the device too (same merges); a tokenizer with any other
        pattern raises MbpeError(ERR_ARG).  "unicode" instead of True: with the splitter's option "unicode", so that
        well-formed non-ASCII text is split there as well (mbpe_tok_set_split_unicode)."""
        text = _u8(data)
        _check(lib().mbpe_tok_set_split_unicode(self._h, int(device_split == "unicode")))
        _check(lib().mbpe_tok_set_train_dedup(self._h, int(bool(dedup))))
        _check(lib().mbpe_tok_set_train_limits(self._h, int(min_frequency), int(max_token_length)))
        if resume:
            _check(lib().mbpe_tok_train_continue(self._h, text.ctypes.data if len(text) else None, len(text), vocab_size,
                                                 conflict_resolution, int(verbose), device, int(bool(device_split))))
            return
        fn = lib().mbpe_tok_train_split_device if device_split else lib().mbpe_tok_train
        _check(fn(self._h, text.ctypes.data if len(text) else None, len(text), vocab_size, conflict_resolution,
                  int(verbose), device))

    def train_from_iterator(self, texts, vocab_size, conflict_resolution=1, verbose=False, device=0, device_split=False,
                            resume=False, repeats=None, min_frequency=0, max_token_length=0):
        """Train on a corpus that arrives in pieces (mbpe_tok_train_pieces_*): every text is split on its own and its
        chunks are counted on the device (mbpe_wordcount_*), then the training runs on the table -- the merges of a
        training on the pieces' chunk lists laid end to end, for both tie-breaks, with one piece in host memory at a
        time.  A piece boundary is a chunk boundary: to get a whole file's result, cut it where a letter or digit is
        followed by whitespace.  repeats: one count per text (default 1), the text counted that many times.
        device_split, resume, min_frequency, max_token_length: as for train().  The tokenizer's merges stay as they are until the training has
        succeeded; the session is aborted when the iterator or a call raises."""
        _check(lib().mbpe_tok_set_split_unicode(self._h, int(device_split == "unicode")))
        _check(lib().mbpe_tok_set_train_limits(self._h, int(min_frequency), int(max_token_length)))
        _check(lib().mbpe_tok_train_pieces_begin(self._h, device, int(bool(device_split))))
        try:
            reps = None if repeats is None else iter(repeats)
            for data in texts:
                text = _u8(data)
                rep = 1 if reps is None else int(next(reps))
                _check(lib().mbpe_tok_train_pieces_add(self._h, text.ctypes.data if len(text) else None, len(text), rep))
            _check(lib().mbpe_tok_train_pieces_finish(self._h, vocab_size, conflict_resolution, int(verbose),
                                                      int(bool(resume))))
        except BaseException:
            lib().mbpe_tok_train_pieces_abort(self._h)
            raise

    def train_files(self, paths, vocab_size, **kw):
        """train_from_iterator over the files' contents, read one at a time."""
        def read():
            for p in paths:
                with open(p, "rb") as f:
                    yield f.read()
        self.train_from_iterator(read(), vocab_size, **kw)

    def _add_pieces(self, texts, repeats):
        reps = None if repeats is None else iter(repeats)
        for data in texts:
            text = _u8(data)
            rep = 1 if reps is None else int(next(reps))
            _check(lib().mbpe_tok_train_pieces_add(self._h, text.ctypes.data if len(text) else None, len(text), rep))

    def _export_pieces(self):
        n = ctypes.c_uint64()
        _check(lib().mbpe_tok_train_pieces_export_size(self._h, ctypes.byref(n)))
        blob = np.zeros(n.value, dtype=np.uint8)
        _check(lib().mbpe_tok_train_pieces_export(self._h, blob.ctypes.data, n.value, ctypes.byref(n)))
        return blob[:n.value].tobytes()

    def count_from_iterator(self, texts, repeats=None, device=0, device_split=False, counts=()):
        """The counting stage of train_from_iterator on its own: the texts are split and their chunks counted on the
        device, and the counts come back as bytes (mbpe_tok_train_pieces_export) -- the word-count table with the
        split pattern and the totals of the verbose lines.  Nothing is trained and the merges are untouched.  Many
        processes, devices or runs can each count a share of the corpus; train_from_counts trains on all of them.
        counts: blobs merged first, in the order given -- how a counting run continues from a checkpoint.  Moving the
        bytes is the caller's business (files, torch.distributed.all_gather_object, MPI)."""
        _check(lib().mbpe_tok_set_split_unicode(self._h, int(device_split == "unicode")))
        _check(lib().mbpe_tok_train_pieces_begin(self._h, device, int(bool(device_split))))
        try:
            for blob in counts:
                b = _u8(blob)
                _check(lib().mbpe_tok_train_pieces_merge(self._h, b.ctypes.data, len(b)))
            self._add_pieces(texts, repeats)
            return self._export_pieces()
        finally:
            lib().mbpe_tok_train_pieces_abort(self._h)

    def count_files(self, paths, **kw):
        """count_from_iterator over the files' contents, read one at a time."""
        def read():
            for p in paths:
                with open(p, "rb") as f:
                    yield f.read()
        return self.count_from_iterator(read(), **kw)

    def train_from_counts(self, blobs, vocab_size, conflict_resolution=1, verbose=False, device=0, resume=False,
                          min_frequency=0, max_token_length=0, texts=None, device_split=False):
        """The training stage on counts made elsewhere: the blobs of count_from_iterator are merged in the order given,
        then any `texts` are added as train_from_iterator adds them (device_split: how these are split), then the
        training runs -- merges, counts, .model, .vocab and verbose lines of train_from_iterator on all the pieces in
        that order, for both tie-breaks.  Blobs given out of piece order train on the pieces in that order: the same
        counts, but the `first` tie-break sees another order of first occurrences.  One rank.  A blob counted under
        another split pattern or one that fails its checks raises MbpeError(ERR_ARG); the merges stay as they are until
        the training has succeeded."""
        _check(lib().mbpe_tok_set_split_unicode(self._h, int(device_split == "unicode")))
        _check(lib().mbpe_tok_set_train_limits(self._h, int(min_frequency), int(max_token_length)))
        _check(lib().mbpe_tok_train_pieces_begin(self._h, device, int(bool(device_split))))
        try:
            for blob in blobs:
                b = _u8(blob)
                _check(lib().mbpe_tok_train_pieces_merge(self._h, b.ctypes.data, len(b)))
            if texts is not None:
                self._add_pieces(texts, None)
            _check(lib().mbpe_tok_train_pieces_finish(self._h, vocab_size, conflict_resolution, int(verbose),
                                                      int(bool(resume))))
        except BaseException:
            lib().mbpe_tok_train_pieces_abort(self._h)
            raise

    def set_merges(self, merges):
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
        _check(lib().mbpe_tok_set_merges(self._h, m.ctypes.data if len(m) else None, len(m)))

    def merges(self):
        n = ctypes.c_uint32()
        _check(lib().mbpe_tok_get_merges(self._h, None, 0, ctypes.byref(n)))
        m = np.zeros((max(n.value, 1), 2), dtype=np.uint32)
        _check(lib().mbpe_tok_get_merges(self._h, m.ctypes.data, n.value, ctypes.byref(n)))
        return m[:n.value]

    def save(self, path, write_vocab=False):
        _check(lib().mbpe_tok_save(self._h, os.fsencode(path), int(write_vocab)))

    def load(self, path, verbose=False):
        _check(lib().mbpe_tok_load(self._h, os.fsencode(path), int(verbose)))

    def _encode_split(self, device_split, order="greedy", dropout=0.0, seed=0, dedup=False, fim=None, mlm=None):
        if order not in ("greedy", "rank"):
            raise ValueError('order must be "greedy" or "rank"')
        _check(lib().mbpe_tok_set_encode_dedup(self._h, int(bool(dedup))))
        _check(lib().mbpe_tok_set_encode_order(self._h, int(order == "rank")))
        _check(lib().mbpe_tok_set_encode_dropout(self._h, dropout_threshold(dropout), int(seed) & 0xFFFFFFFFFFFFFFFF))
        _check(lib().mbpe_tok_set_encode_split(self._h, int(bool(device_split))))
        _check(lib().mbpe_tok_set_split_unicode(self._h, int(device_split == "unicode")))
        _check(lib().mbpe_tok_set_encode_fim(self._h, None if fim is None else ctypes.byref(fim)))
        _check(lib().mbpe_tok_set_encode_mlm(self._h, None if mlm is None else ctypes.byref(mlm)))

    def fim_info(self):
        """The fill-in-the-middle plan of the latest batch call with a device (mbpe_tok_encode_fim_info) -> (mode
        uint8[n_texts], cuts uint64[n_texts, 2]): FIM_NONE / FIM_PSM / FIM_SPM and the cuts (a, b) of every text."""
        return _fim_info(lib().mbpe_tok_encode_fim_info, self._h)

    def encode(self, data, device=None, device_split=False, order="greedy", byte_ranges=False, dropout=0.0, seed=0,
               dedup=False):
        """device None: internal_encode on the host; an int: on that HIP device (mbpe_tok_encode_device).
        device_split (here and in the batch calls; only with a device): the text is cut at the special tokens and split
        into chunks on the device too (mbpe_tok_set_encode_split); same tokens, gpt2 / gpt4 patterns only.  "unicode"
        instead of True: with the splitter's option "unicode" for that call (mbpe_tok_set_split_unicode).
        order (here and in the batch calls; host and device): "greedy", the reference's passes that replace any pair
        they find, or "rank": a chunk's pair with the lowest merge id first, which for a trained model is the
        segmentation the trainer left in its stream (mbpe_tok_set_encode_order).  Anything else is ValueError.
        dropout, seed (here and in the batch calls; host and device; mbpe_tok_set_encode_dropout): BPE-dropout, a merge
        instance is skipped with probability dropout, decided by a hash of (seed, byte position, merged id); only with
        order="rank" -- with "greedy" and dropout > 0 the library's error is raised.  Positions are those of the
        buffer the route hands the encoder, so the host loop and the device over the host split always agree, and
        they agree with device_split when the text has no special token and the pattern is basic, gpt2 or gpt4.
        byte_ranges=True (mbpe_tok_encode_byteoff): -> (tokens, ranges[n, 2] uint64), token j stands for
        data[ranges[j, 0]:ranges[j, 1]] (a special token: the occurrence of its name).
        dedup=True (here and in the batch calls; only with a device; mbpe_tok_set_encode_dedup): the chunks are
        deduplicated on the device, the distinct ones encoded once and their tokens copied to every occurrence; same
        tokens.  With byte_ranges or dropout > 0 the library's error is raised."""
        self._encode_split(device_split, order, dropout, seed, dedup)
        text = _u8(data)
        n = ctypes.c_uint64()
        out = np.zeros(max(len(text), 1), dtype=np.uint32)
        if byte_ranges:
            ranges = np.zeros((len(out), 2), dtype=np.uint64)
            _check(lib().mbpe_tok_encode_byteoff(self._h, text.ctypes.data if len(text) else None, len(text), 0,
                                                 -1 if device is None else device, out.ctypes.data, ranges.ctypes.data,
                                                 len(out), ctypes.byref(n)))
            return out[:n.value].copy(), ranges[:n.value].copy()
        if device is None:
            _check(lib().mbpe_tok_encode(self._h, text.ctypes.data if len(text) else None, len(text), 0,
                                         out.ctypes.data, len(out), ctypes.byref(n)))
        else:
            _check(lib().mbpe_tok_encode_device(self._h, text.ctypes.data if len(text) else None, len(text), 0, device,
                                                out.ctypes.data, len(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def encode_batch(self, texts, device=0, device_split=False, order="greedy", byte_ranges=False, dropout=0.0,
                     seed=0, dedup=False):
        """encode() of every text in one device call (mbpe_tok_encode_batch_device) -> list of uint32 arrays; with
        byte_ranges=True (mbpe_tok_encode_batch_byteoff_device) a list of (tokens, ranges[n, 2] uint64) pairs, the
        ranges relative to each text's first byte.  With dropout, positions run over the texts laid end to end."""
        self._encode_split(device_split, order, dropout, seed, dedup)
        parts = [bytes(_u8(t)) for t in texts]
        doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        out = np.zeros(max(len(text), 1), dtype=np.uint32)
        tok_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        if byte_ranges:
            ranges = np.zeros((len(out), 2), dtype=np.uint64)
            _check(lib().mbpe_tok_encode_batch_byteoff_device(self._h, text.ctypes.data if len(text) else None,
                                                              doc_off.ctypes.data, len(parts), 0, device, out.ctypes.data,
                                                              ranges.ctypes.data, len(out), tok_off.ctypes.data,
                                                              ctypes.byref(n)))
            return [(out[int(a):int(b)].copy(), ranges[int(a):int(b)].copy()) for a, b in zip(tok_off[:-1], tok_off[1:])]
        _check(lib().mbpe_tok_encode_batch_device(self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data,
                                                  len(parts), 0, device, out.ctypes.data, len(out), tok_off.ctypes.data,
                                                  ctypes.byref(n)))
        return [out[int(a):int(b)].copy() for a, b in zip(tok_off[:-1], tok_off[1:])]

    def token_counts(self, texts, device=0, device_split=False, order="greedy", dropout=0.0, seed=0, dedup=False,
                     repeats=None, batch_bytes=1 << 28):
        """How often every token id is used on `texts` (any iterable of texts) -> uint64[n_ids], n_ids = max(256 +
        merges, largest special id + 1): the bincount of encode() of every text, text i counted repeats[i] times
        (mbpe_tok_count_tokens).  With a device no token leaves it: the texts go there in batches of whole texts of at
        most batch_bytes (a longer text is a batch of its own), and only the table comes back.  device=None is the host
        loop.  device_split, order, dropout, seed and dedup as for encode_batch.  The table is reset first."""
        self._encode_split(device_split, order, dropout, seed, dedup)
        _check(lib().mbpe_tok_token_counts_reset(self._h))
        dev = -1 if device is None else device

        def flush(parts, rep):
            doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
            text = np.frombuffer(b"".join(parts), dtype=np.uint8)
            n = ctypes.c_uint64()
            _check(lib().mbpe_tok_count_tokens(self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data,
                                               len(parts), 0, dev, rep, ctypes.byref(n)))

        reps = None if repeats is None else iter(repeats)
        parts, held, cur = [], 0, 1
        for data in texts:
            part = bytes(_u8(data))
            rep = 1 if reps is None else int(next(reps))
            if parts and (rep != cur or held + len(part) > batch_bytes):
                flush(parts, cur)
                parts, held = [], 0
            parts.append(part)
            held, cur = held + len(part), rep
        if parts:
            flush(parts, cur)
        n_ids = ctypes.c_uint64()
        _check(lib().mbpe_tok_token_counts(self._h, None, 0, ctypes.byref(n_ids), None))
        out = np.zeros(n_ids.value, dtype=np.uint64)
        _check(lib().mbpe_tok_token_counts(self._h, out.ctypes.data, len(out), ctypes.byref(n_ids), None))
        return out

    def encode_batch_padded(self, texts, seq_len, layout="padded", out_bits=32, pad_id=0, bos_id=None, eos_id=None,
                            pad_left=False, trunc_left=False, device=0, out_ptr=None, len_ptr=None, cap_rows=None,
                            device_split=False, order="greedy", dropout=0.0, seed=0, dedup=False, fim=None):
        """Every text split like encode(), encoded and packed in one device call
        (mbpe_tok_encode_batch_packed_device) -> (ids [n_rows, seq_len], lengths [n_rows]) as numpy arrays; with
        out_ptr= and len_ptr= (device memory for cap_rows rows) the matrix stays on the device and the row count is
        returned.  bos_id / eos_id may be special-token ids.  layout "packed" gives the MBPE_PACK_PACKED rows.
        fim (here and in _aux, _windows and _fit; mbpe_tok_set_encode_fim): a FimSpec (fim_spec()) -- every text's
        tokens go through the fill-in-the-middle transform on the device before they are packed; its sentinel ids may
        be special-token ids; fim_info() tells what was done to each text.  With "padded" rows and truncation a
        transformed text that does not fit loses its middle: use max_tokens, windows, "packed" or fit there."""
        self._encode_split(device_split, order, dropout, seed, dedup, fim)
        spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
        parts = [bytes(_u8(t)) for t in texts]
        doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
        head = (self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data, len(parts), 0, device,
                ctypes.byref(spec))
        tail = (ctypes.byref(n_rows), ctypes.byref(n_tok))
        if out_ptr is not None:
            _check(lib().mbpe_tok_encode_batch_packed_device(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail))
            return n_rows.value
        if spec.layout == PACK_PADDED:
            n_rows.value = len(parts)
        else:
            _check(lib().mbpe_tok_encode_batch_packed_device(*head, None, 0, 0, None, *tail))
        ids, lengths = _matrix(n_rows.value, spec)
        _check(lib().mbpe_tok_encode_batch_packed_device(*head, ids.ctypes.data if ids.size else None, len(ids), 0,
                                                         lengths.ctypes.data if len(ids) else None, *tail))
        return ids, lengths

    def encode_batch_denoise(self, texts, enc_len, dec_len, denoise, device=0, out_bits=32, pad_id=0, eos_id=None,
                             decoder_start_id=None, ignore_label=-100, labels=True, row_doc=True, ptrs=None,
                             cap_rows=None, device_split=False, order="greedy", dropout=0.0, seed=0, dedup=False):
        """Every text split like encode(), encoded, span-corrupted (T5 / UL2; denoise: a DenoiseSpec from
        denoise_spec()) and packed into the two matrices of an encoder-decoder batch in one device call
        (mbpe_tok_encode_batch_denoise_device) -> the dict of Encoder.encode_batch_denoise, as numpy arrays or -- ptrs=,
        cap_rows= -- written into device memory such as torch tensors, the row count returned (self.n_rows holds it
        also where cap_rows is too small).  One row per unit: with denoise.segment_tokens a long text becomes several
        rows and "row_doc" says whose.  eos_id, decoder_start_id and the sentinels may be special-token ids.  The
        tokens encoded: self.n_tokens."""
        self._encode_split(device_split, order, dropout, seed, dedup)
        es, ds = _denoise_specs(enc_len, dec_len, out_bits, pad_id, eos_id, decoder_start_id)
        parts = [bytes(_u8(t)) for t in texts]
        doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        fn = lib().mbpe_tok_encode_batch_denoise_device

        def call(batch, cap, on_dev):
            n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
            rc = fn(self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data, len(parts), 0, device,
                    ctypes.byref(denoise), ctypes.byref(es), ctypes.byref(ds), batch, cap, on_dev, ctypes.byref(n_rows),
                    ctypes.byref(n_tok))
            return rc, n_rows.value, n_tok.value
        rc, out, self.n_tokens = _denoise_batch(call, len(parts), denoise, es, ds, ignore_label, ptrs, cap_rows, labels,
                                                row_doc)
        if isinstance(out, int):
            self.n_rows = out
        _check(rc)
        return out

    def encode_batch_aux(self, texts, seq_len, layout="padded", out_bits=32, pad_id=0, bos_id=None, eos_id=None,
                         pad_left=False, trunc_left=False, device=0, out_ptr=None, len_ptr=None, cap_rows=None,
                         labels=False, positions=False, segments=False, cu_seqlens=False, ignore_label=-100,
                         labels_ptr=None, pos_ptr=None, seg_ptr=None, device_split=False, order="greedy", dropout=0.0,
                         seed=0, dedup=False, fim=None, mlm=None):
        """encode_batch_padded plus labels, positions, segments and cu_seqlens (mbpe_tok_encode_batch_aux_device): its
        arguments and those of pack_tokens_aux, whose dict (or, with out_ptr=, row count) is returned.  The documents'
        token offsets of the call (with fim: after the transform): self.doc_tok_off.
        mlm (here and in _windows and _fit; mbpe_tok_set_encode_mlm): an MlmSpec (mlm_spec()) -- every text's tokens go
        through masked-LM corruption on the device before they are packed: "ids" are the corrupted ids, "labels" the
        targets (ignore_label in every other cell).  whole_word masks the chunks of the split pattern as wholes and
        needs out_bits 32 or 64.  Not together with fim."""
        self._encode_split(device_split, order, dropout, seed, dedup, fim, mlm)
        spec = pack_spec(seq_len, layout, out_bits, pad_id, bos_id, eos_id, pad_left, trunc_left)
        call = _AuxCall(spec, labels, positions, segments, cu_seqlens, ignore_label)
        parts = [bytes(_u8(t)) for t in texts]
        doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        n_rows, n_tok = ctypes.c_uint64(), ctypes.c_uint64()
        doc_tok_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        head = (self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data, len(parts), 0, device,
                ctypes.byref(spec))
        tail = (ctypes.byref(n_rows), ctypes.byref(n_tok))
        fn = lib().mbpe_tok_encode_batch_aux_device
        if out_ptr is not None:
            aux = call.device(labels_ptr, pos_ptr, seg_ptr)
            _check(fn(*head, _ptr(out_ptr), cap_rows or 0, 1, _ptr(len_ptr), *tail, ctypes.byref(aux),
                      doc_tok_off.ctypes.data))
            self.doc_tok_off = doc_tok_off
            return (n_rows.value,) + call.cu_seqlens(doc_tok_off) if cu_seqlens else n_rows.value
        if spec.layout == PACK_PADDED:
            n_rows.value = len(parts)
        else:
            aux = call.device(None, None, None)
            _check(fn(*head, None, 0, 0, None, *tail, ctypes.byref(aux), None))
        ids, lengths = _matrix(n_rows.value, spec)
        aux, arrays = call.host(n_rows.value)
        _check(fn(*head, ids.ctypes.data if ids.size else None, len(ids), 0, lengths.ctypes.data if len(ids) else None,
                  *tail, ctypes.byref(aux), doc_tok_off.ctypes.data))
        self.doc_tok_off = doc_tok_off
        return call.result(ids, lengths, arrays, doc_tok_off)

    def encode_batch_windows(self, texts, seq_len, stride, score_once=False, out_bits=32, pad_id=0, bos_id=None,
                             eos_id=None, device=0, out_ptr=None, len_ptr=None, cap_rows=None, labels=False,
                             positions=False, segments=False, ignore_label=-100, labels_ptr=None, pos_ptr=None,
                             seg_ptr=None, row_doc=False, row_tok0=False, row_doc_ptr=None, row_tok0_ptr=None,
                             device_split=False, order="greedy", dropout=0.0, seed=0, dedup=False, fim=None,
                             mlm=None):
        """encode_batch_aux for the window layout (mbpe_tok_encode_batch_windows_device): every text split like
        encode(), encoded, and cut into rows of seq_len that share `stride` tokens where a text does not fit one --
        the keywords and the result of pack_windows ("row_doc" maps a row back to its text).  The texts' token
        offsets of the call: self.doc_tok_off."""
        self._encode_split(device_split, order, dropout, seed, dedup, fim, mlm)
        spec = pack_spec(seq_len, "padded", out_bits, pad_id, bos_id, eos_id)
        call = _WinCall(spec, stride, score_once, labels, positions, segments, ignore_label, row_doc, row_tok0)
        parts = [bytes(_u8(t)) for t in texts]
        doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        n_tok = ctypes.c_uint64()
        doc_tok_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        head = (self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data, len(parts), 0, device,
                ctypes.byref(spec))
        tail = lambda n_rows, aux, win: (ctypes.byref(n_rows), ctypes.byref(n_tok), ctypes.byref(aux),
                                         doc_tok_off.ctypes.data, ctypes.byref(win))
        out = call.run(lib().mbpe_tok_encode_batch_windows_device, head, tail, out_ptr, len_ptr, cap_rows,
                       (labels_ptr, pos_ptr, seg_ptr, row_doc_ptr, row_tok0_ptr))
        self.doc_tok_off = doc_tok_off
        return out

    def encode_batch_fit(self, texts, seq_len, out_bits=32, pad_id=0, bos_id=None, eos_id=None, device=0, out_ptr=None,
                         len_ptr=None, cap_rows=None, labels=False, positions=False, segments=False, cu_seqlens=False,
                         ignore_label=-100, labels_ptr=None, pos_ptr=None, seg_ptr=None, doc_row=False, doc_col=False,
                         doc_row_ptr=None, doc_col_ptr=None, device_split=False, order="greedy", dropout=0.0, seed=0,
                         dedup=False, fim=None, mlm=None):
        """encode_batch_aux for the fit layout (mbpe_tok_encode_batch_fit_device): every text split like encode(),
        encoded, and packed whole into rows of seq_len by best fit; only a text longer than a row is cut -- the
        keywords and the result of pack_fit ("doc_row" / "doc_col" say where a text's last piece begins, "segments"
        holds the text's number + 1 in every cell).  The texts' token offsets of the call: self.doc_tok_off."""
        self._encode_split(device_split, order, dropout, seed, dedup, fim, mlm)
        spec = _fit_spec(seq_len, out_bits, pad_id, bos_id, eos_id)
        call = _FitCall(spec, labels, positions, segments, cu_seqlens, ignore_label, doc_row, doc_col)
        parts = [bytes(_u8(t)) for t in texts]
        doc_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            doc_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8)
        n_tok = ctypes.c_uint64()
        doc_tok_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        head = (self._h, text.ctypes.data if len(text) else None, doc_off.ctypes.data, len(parts), 0, device,
                ctypes.byref(spec))
        tail = lambda n_rows, aux, fit: (ctypes.byref(n_rows), ctypes.byref(n_tok), ctypes.byref(aux),
                                         doc_tok_off.ctypes.data, ctypes.byref(fit))
        out = call.run(lib().mbpe_tok_encode_batch_fit_device, head, tail, len(parts), lambda: doc_tok_off, out_ptr,
                       len_ptr, cap_rows, (labels_ptr, pos_ptr, seg_ptr, doc_row_ptr, doc_col_ptr))
        self.doc_tok_off = doc_tok_off
        return out

    def decode_padded(self, ids, lengths, device=0):
        """A right-padded id matrix [n_rows, seq_len] and its lengths -> the list of the rows' texts, unpacked and
        decoded on the device (mbpe_tok_decode_padded_device); the mirror of encode_batch_padded."""
        m = np.ascontiguousarray(ids, dtype=np.uint32)
        n_rows, seq_len = m.shape
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        if len(ln) != n_rows:
            raise ValueError("one length per row")
        byte_off = np.zeros(n_rows + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        args = (self._h, m.ctypes.data if m.size else None, n_rows, seq_len, ln.ctypes.data if n_rows else None, 0, device)
        _check(lib().mbpe_tok_decode_padded_device(*args, None, 0, byte_off.ctypes.data, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_tok_decode_padded_device(*args, out.ctypes.data, len(out), byte_off.ctypes.data, ctypes.byref(n)))
        data = out[:n.value].tobytes()
        return [data[int(a):int(b)] for a, b in zip(byte_off[:-1], byte_off[1:])]

    def decode(self, tokens, device=None):
        """device None: the host loop; an int: on that HIP device (mbpe_tok_decode_device)."""
        t = np.ascontiguousarray(tokens, dtype=np.uint32)
        tp = t.ctypes.data if len(t) else None
        n = ctypes.c_uint64()
        if device is None:
            _check(lib().mbpe_tok_decode(self._h, tp, len(t), 0, None, 0, ctypes.byref(n)))
            out = np.zeros(max(n.value, 1), dtype=np.uint8)
            _check(lib().mbpe_tok_decode(self._h, tp, len(t), 0, out.ctypes.data, len(out), ctypes.byref(n)))
            return out[:n.value].tobytes()
        _check(lib().mbpe_tok_decode_device(self._h, tp, len(t), 0, device, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_tok_decode_device(self._h, tp, len(t), 0, device, out.ctypes.data, len(out), ctypes.byref(n)))
        return out[:n.value].tobytes()

    def decode_batch(self, token_lists, device=0):
        """decode() of every token list in one device call each for the lengths and the bytes
        (mbpe_tok_decode_batch_device) -> list of bytes; the mirror of encode_batch."""
        parts = [np.ascontiguousarray(t, dtype=np.uint32).reshape(-1) for t in token_lists]
        tok_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            tok_off[1:] = np.cumsum([len(t) for t in parts], dtype=np.uint64)
        t = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
        tp = t.ctypes.data if len(t) else None
        byte_off = np.zeros(len(parts) + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        args = (self._h, tp, tok_off.ctypes.data, len(parts), 0, device)
        _check(lib().mbpe_tok_decode_batch_device(*args, None, 0, byte_off.ctypes.data, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mbpe_tok_decode_batch_device(*args, out.ctypes.data, len(out), byte_off.ctypes.data, ctypes.byref(n)))
        data = out[:n.value].tobytes()
        return [data[int(a):int(b)] for a, b in zip(byte_off[:-1], byte_off[1:])]
