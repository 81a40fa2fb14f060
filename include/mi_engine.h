/* mi_engine.h -- C ABI of the MI355X-native quantized-inference engine.
 *
 * This is the drop-in boundary for Blama's hot path.  Blama's inference layer
 * (bl::llama, /root/reference/inference/code/llama) binds the llama.cpp C API
 * (llama.h, llama.cpp tag b5187); the entry points below replace the hot-path
 * subset of it.  Each declaration cites the reference call
 * site whose llama.h function it replaces.
 *
 * Conventions: plain C types only; functions returning pointers return NULL on
 * error and functions returning int32_t return a negative value on error, with
 * the message available from mi_last_error() (thread-local).  mi_decode keeps
 * llama_decode's convention: 0 = ok, 1 = no KV space, < 0 = error
 * (checked "!= 0" at Session.cpp:388).  One context is used by one thread at a
 * time (Server.cpp:36); a model may back several contexts.
 */
#ifndef MI_ENGINE_H
#define MI_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_model mi_model;
typedef struct mi_ctx mi_ctx;

typedef struct mi_model_params {
    int32_t device_ordinal; /* HIP device; Model.cpp:18-21 binds the first GPU */
    int32_t cpu_only;       /* Model::Params::gpu=false -- not served here: returns NULL */
    int32_t vocab_only;     /* Model::Params::vocabOnly: parse metadata/vocab, no weights */
    int32_t no_upload;      /* allocate the weight arena but leave it unfilled (replica
                               that receives the weights by RCCL broadcast) */
} mi_model_params;

/* Last error message of this thread ("" if none). */
const char* mi_last_error(void);

/* ---- model: replaces llama_model_load_from_file / llama_model_free
 *      (Model.cpp:52, Model.hpp:55) ---- */
/* Weight types served: quantised models (layer matrices, output head and token_embd each one of
 * Q4_K / Q5_K / Q6_K / Q8_0 and, in a dense LLaMA-graph model, Q4_0 / Q5_0: llama-quantize's Q4_0 and
 * Q5_0 files -- head Q6_K -- and the tensors it stores as Q4_0 / Q5_0 inside a k-quant file; Q4_0 and
 * Q5_0 matrices take Q8_0 activations as Q8_0 ones do.  Refused with the tensor and the type by name,
 * vocab_only included: Q4_1, Q5_1 (Q8_1 activations), Q2_K, Q3_K, the IQ and TQ types, and a Q4_0 /
 * Q5_0 matrix in a MoE, GPT-2 or BERT model),
 * BERT encoders (F16), and unquantised dense LLaMA-graph models (general.architecture "llama",
 * no experts) whose matrices -- token_embd, output and the seven per layer -- are all F16 with F32
 * norm weights and rope_freqs; without output.weight the head is token_embd (tied models such as
 * Llama-3.2).  Shape rules of an F16 model: embedding_length = head_count x head_dim, head_count a
 * multiple of head_count_kv; embedding_length and feed_forward_length multiples of 32, at most
 * 16384; head_count_kv x head_dim and the vocabulary size multiples of 32; rope.dimension_count
 * even.  Refused at load (vocab_only included), each with a message naming the tensor and the
 * reason: BF16 matrices, F32 matrices, a file mixing F16 and quantised matrices, F16 MoE, F16
 * GPT-2, a shape outside the rules.  mi_lora_load and mi_ctx_set_lora refuse an F16 base model:
 * LoRA on unquantised models is not implemented. */
mi_model* mi_model_load(const char* gguf_path, const mi_model_params* params);
/* Same, from a GGUF image in host memory (with no_upload/vocab_only only the
 * header -- metadata and tensor infos -- needs to be present). */
mi_model* mi_model_load_from_memory(const void* data, size_t size, const mi_model_params* params);
void mi_model_free(mi_model* model);

/* hparams / vocab queries: llama_vocab_n_tokens (Session.cpp:27),
 * llama_model_n_ctx_train (Model.cpp:41), llama_vocab_bos/eos (Instance.cpp:91-92),
 * llama_vocab_get_add_bos (Model.cpp:45), llama_model_meta_val_str (Model.cpp:57) */
int32_t mi_model_n_vocab(const mi_model* model);
int32_t mi_model_n_ctx_train(const mi_model* model);
int32_t mi_model_n_embd(const mi_model* model);
int32_t mi_model_n_layer(const mi_model* model);
int32_t mi_model_n_head(const mi_model* model);
int32_t mi_model_n_head_kv(const mi_model* model);
int32_t mi_model_n_ff(const mi_model* model);
int32_t mi_model_n_expert(const mi_model* model);
/* llama_model_rope_freq_scale_train: 1 / the linear RoPE scaling factor (1 when unscaled) */
float mi_model_rope_freq_scale(const mi_model* model);
int32_t mi_model_token_bos(const mi_model* model);
int32_t mi_model_token_eos(const mi_model* model);
int32_t mi_model_add_bos(const mi_model* model);
int32_t mi_model_token_is_eog(const mi_model* model, int32_t token);
/* Text of a vocabulary entry (raw GGUF piece); returns its length or < 0. */
int32_t mi_model_token_text(const mi_model* model, int32_t token, char* buf, int32_t size);
/* Vocabulary for the host tokenizer (Vocab.cpp:37-72 -> llama_tokenize / llama_token_to_piece):
 * entries in tokenizer.ggml.tokens, SPM merge score, llama_token_type (1 normal, 2 unknown,
 * 3 control, 4 user-defined, 5 unused, 6 byte), and tokenizer.ggml.model ("llama" = SPM). */
int32_t mi_model_n_tokens(const mi_model* model);
float mi_model_token_score(const mi_model* model, int32_t token);
int32_t mi_model_token_type(const mi_model* model, int32_t token);
int32_t mi_model_tokenizer(const mi_model* model, char* buf, int32_t size);
int32_t mi_model_meta_str(const mi_model* model, const char* key, char* buf, int32_t size);
/* BPE vocabularies (tokenizer.ggml.model "gpt2", e.g. Llama-3): tokenizer.ggml.merges, rank = index;
 * mi_model_merge returns the length of merge i ("left right") or < 0. */
int32_t mi_model_n_merges(const mi_model* model);
int32_t mi_model_merge(const mi_model* model, int32_t i, char* buf, int32_t size);
/* Bytes of weights a decode step streams (all tensors but tok_embd -- included when it is also the
 * output head; of an MoE expert tensor only the n_expert_used experts a token is routed to); for
 * an F16 model the F16 bytes. */
int64_t mi_model_weight_bytes(const mi_model* model);
/* The device weight arena (one allocation) -- for the replica broadcast. */
int32_t mi_model_arena(const mi_model* model, void** dev_ptr, size_t* bytes);
/* Replicas for concurrent sessions (one worker per replica, Server.cpp:36): fills
 * the weight arenas of models[1..n-1] -- each loaded from the same GGUF with no_upload, i.e. the
 * header only -- from models[0].  Devices other than models[0]'s receive the arena by one RCCL
 * broadcast over xGMI (ncclCommInitAll over the distinct devices, root models[0]); further
 * replicas on a device take a device-to-device copy.  Call before any mi_ctx_create on the
 * replicas (their prompt-batch weight copies are built from the arena then).  0 ok, < 0 error. */
int32_t mi_model_replicate(mi_model* const* models, int32_t n);
/* Per ggml type id (0..31): bytes of weights of that type (the GGUF's byte histogram). */
int32_t mi_model_type_histogram(const mi_model* model, int64_t* bytes_by_type, int32_t n);

/* ---- context: replaces llama_init_from_model / llama_free (Instance.cpp:36);
 *      n_ctx 0 = training context (Instance.hpp:22) ---- */
mi_ctx* mi_ctx_create(mi_model* model, uint32_t n_ctx, uint32_t n_batch, uint32_t n_ubatch);
void mi_ctx_free(mi_ctx* ctx);
uint32_t mi_n_ctx(const mi_ctx* ctx);     /* llama_n_ctx   (Session.cpp:57,72,162,322) */
uint32_t mi_n_batch(const mi_ctx* ctx);   /* llama_n_batch (Session.cpp:381) */

/* llama_decode(llama_batch_get_one(tokens, n)) (Session.cpp:388, Instance.cpp:115):
 * tokens take positions pos_max+1...; asynchronous on the context's stream.
 * out_mode MI_OUT_LAST = logits of the last token only (llama_batch_get_one);
 * MI_OUT_ALL = logits of every token (a batch with logits[i] = true for all i), n <= n_batch:
 * output row i is the distribution after token i -- one batched pass in place of the
 * per-token decodes of Session::fillCtx (Session.cpp:231-244). */
#define MI_OUT_LAST 0
#define MI_OUT_ALL 1
int32_t mi_decode(mi_ctx* ctx, const int32_t* tokens, int32_t n, int32_t out_mode);

/* Output rows: -1 = the last token's; 0..n-1 after an MI_OUT_ALL decode of n tokens (row 0 only
 * after MI_OUT_LAST).  Top-k of an output row, sorted by logit descending then id ascending;
 * k <= 64.  Replaces fillLogits + std::sort + first 10 (Session.cpp:246-261) and
 * feeds the sampler chain's top_k(40) stage (Sampler.cpp:15-97).  Synchronises. */
int32_t mi_topk(mi_ctx* ctx, int32_t row, int32_t k, int32_t* ids, float* logits);
/* Logits of an output row at the given ids (Session.cpp:263-282).  Synchronises. */
int32_t mi_gather(mi_ctx* ctx, int32_t row, const int32_t* ids, int32_t n, float* out);
/* Batched form of mi_gather for a verification pass: rows row0 .. row0+n_rows-1, k ids per row
 * (ids and out are [n_rows][k]).  Returns n_rows*k or < 0.  Synchronises. */
int32_t mi_gather_rows(mi_ctx* ctx, int32_t row0, int32_t n_rows, const int32_t* ids, int32_t k, float* out);
/* Full-vocabulary escape hatch: llama_get_logits_ith(ctx, -1) (Session.cpp:24,
 * Sampler.cpp:111).  Context-owned; valid until the next decode.  Synchronises. */
const float* mi_logits(mi_ctx* ctx, int32_t row);
void mi_synchronize(mi_ctx* ctx);         /* llama_synchronize (Session.cpp:54) */

/* KV cache (single sequence): llama_kv_self_clear (Session.cpp:53),
 * llama_kv_self_seq_rm / seq_add / seq_div (Session.cpp:341-342, 359-361).
 * p1 < 0 means "to the end". */
void mi_kv_clear(mi_ctx* ctx);
int32_t mi_kv_seq_rm(mi_ctx* ctx, int32_t p0, int32_t p1);
int32_t mi_kv_seq_add(mi_ctx* ctx, int32_t p0, int32_t p1, int32_t delta);
int32_t mi_kv_seq_div(mi_ctx* ctx, int32_t p0, int32_t p1, int32_t d);
int32_t mi_kv_pos_max(const mi_ctx* ctx); /* -1 when empty */
int32_t mi_kv_n_cells(const mi_ctx* ctx);

/* State save/restore: llama_state_get_size / get_data / set_data (Session.cpp:291-304). */
size_t mi_state_size(mi_ctx* ctx);
size_t mi_state_get(mi_ctx* ctx, uint8_t* dst, size_t size);
size_t mi_state_set(mi_ctx* ctx, const uint8_t* src, size_t size);

/* Control vectors: llama_apply_adapter_cvec (Instance.cpp:74-79, Instance::addControlVector).
 * data holds the directions of layers 1, 2, ... back to back (len floats, n_embd each; layer 0 has
 * none).  Layer il (0-based) gets data[(il-1)*n_embd ..) added to its output -- after the FFN
 * residual add, llm_build_llama / llm_build_gpt2's build_cvec -- when 1 <= il <= n_layer-1,
 * il_start <= il <= il_end and il*n_embd <= len; every other layer gets nothing.  data NULL
 * switches the vector off.  The vector belongs to the context (not to mi_state_get / mi_state_set),
 * takes effect from the next mi_decode and leaves the KV entries of earlier tokens as they are.
 * Synchronises.  0 ok; < 0 error (n_embd differs from the model's, null context). */
int32_t mi_ctx_apply_cvec(mi_ctx* ctx, const float* data, size_t len, int32_t n_embd, int32_t il_start,
                          int32_t il_end);
/* The control-vector file loader (ControlVector.cpp:20-98, loadControlVector): every tensor of the
 * GGUF must be named direction.N (N >= 1), F32 and 1-D, all of one length n_embd;
 * data[n_embd*(N-1) + j] += src[j] * strength (tensors of one N accumulate, and so do several
 * files loaded into one zero-initialised buffer: ControlVector.cpp:105-127).  Returns the floats
 * needed, n_embd * max N, and writes data only when cap (floats) is at least that; data NULL is a
 * size query.  *n_embd (optional) receives the tensors' length.  < 0: unreadable file, a tensor
 * that is not direction.N with N >= 1, not F32, not 1-D, or of another length than the first. */
int64_t mi_cvec_load(const char* gguf_path, float strength, float* data, size_t cap, int32_t* n_embd);

/* LoRA adapters (llama.cpp b5187 src/llama-adapter.cpp, llama-graph.cpp build_lora_mm): for every
 * base tensor W an adapter holds, y = W cur + s * (B (A cur)) with s = scale * alpha / r (alpha 0:
 * s = scale), ahead of everything downstream (RoPE, the KV append, SwiGLU, the residual add).
 * Dense LLaMA models; the per-layer attn_q/k/v/output and ffn_gate/up/down tensors; F16 or F32
 * adapter tensors; rank 1..128 per pair, at most 4 adapters on a context with a summed rank of at
 * most 128 per base tensor.
 *
 * mi_lora_load / _from_memory: llama_adapter_lora_init (LoraAdapter.cpp:12-19).  NULL and
 * mi_last_error() when general.type is not "adapter" or adapter.type not "lora", the architecture
 * differs from the model's, a tensor name ends in neither .lora_a nor .lora_b, a pair lacks a
 * half, the base tensor does not exist in the model or is not one of the seven above, a shape does
 * not fit (invalid shape, not transposed), a type is neither F16 nor F32, the rank is above 128,
 * the model is MoE or GPT-2, or the file is truncated.  On a vocab_only model the file is parsed
 * and validated only.  The adapter is shared-owned: a context keeps what it was given alive, so
 * mi_lora_free on an adapter still set on a context is safe. */
typedef struct mi_lora mi_lora;
mi_lora* mi_lora_load(mi_model* model, const char* gguf_path);
mi_lora* mi_lora_load_from_memory(mi_model* model, const void* data, size_t size);
void mi_lora_free(mi_lora* lora);
float mi_lora_alpha(const mi_lora* lora);
int32_t mi_lora_n_pairs(const mi_lora* lora);
/* llama_set_adapter_lora (Instance.cpp:52-57, Instance::addLora): adds the adapter to the context
 * or updates its scale; adapters stack.  mi_ctx_rm_lora: llama_rm_adapter_lora, 0 or < 0 when the
 * adapter is not set.  mi_ctx_clear_lora: llama_clear_adapter_lora (Instance.cpp:59-61,
 * Instance::clearLoraState).  Like the control vector the adapters belong to the context (not to
 * mi_state_get / mi_state_set), take effect from the next mi_decode and leave the KV entries of
 * earlier tokens as they are; the calls synchronise.  < 0: a null argument, an adapter of another
 * model (Instance.cpp:53-55), a fifth adapter or a summed rank above 128. */
int32_t mi_ctx_set_lora(mi_ctx* ctx, mi_lora* lora, float scale);
int32_t mi_ctx_rm_lora(mi_ctx* ctx, mi_lora* lora);
void mi_ctx_clear_lora(mi_ctx* ctx);

/* Embeddings (InstanceEmbedding.cpp:24-32: llama_context_params.embeddings = true, pooling_type;
 * InstanceEmbedding.cpp:113-164: llama_decode, llama_pooling_type, llama_get_embeddings_ith /
 * llama_get_embeddings_seq).  The embedding of a token is result_norm: the residual stream after the
 * last layer (its control-vector add and any LoRA included) through the final norm, in f32 --
 * rms_norm(x) * output_norm (LLaMA, MoE), layer_norm(x) * output_norm + bias (GPT-2).  Pooling
 * (llama_pooling_type) reduces the rows of the tokens of ONE mi_decode call (n <= n_batch) to one
 * row: MEAN = sum_t row_t * (1.0f / n) in f32 in token order, CLS = the first token's row, LAST =
 * the last token's; NONE keeps a row per output token.  RANK needs a classification head the engine
 * does not load and is refused.
 *
 * Encoder models (general.architecture "bert": BERT-architecture F16 models such as the bge family,
 * head_dim 32 or 64; llm_build_bert).  A context on one holds no KV cache and is ALWAYS in
 * embeddings mode, created with the model's pooling type (NONE when the key is absent).  Every
 * mi_decode call is one stateless bidirectional pass: its n tokens take positions 0 .. n - 1, use
 * token type 0 and attend to each other only; n <= min(n_batch, 512, n_ctx_train), more is refused
 * (< 0, with a message), as are token ids outside the vocabulary.  out_mode, pooling and the rows of
 * mi_embeddings are as above.  On such a context: mi_ctx_set_embeddings(ctx, 0, ..) < 0 (no output
 * head); mi_kv_pos_max is -1 and mi_kv_n_cells 0 always; mi_kv_clear is a no-op; mi_kv_seq_* and
 * mi_ctx_apply_cvec < 0; mi_state_size / mi_state_get / mi_state_set return 0; mi_logits NULL,
 * mi_topk / mi_gather / mi_gather_rows < 0; mi_lora_load on the model is refused.  Not served:
 * quantised or F32 BERT matrices, the nomic / jina variants (RoPE, gated FFN, attention-norm
 * tensors), RANK pooling, token types other than 0, several sequences in one call. */
#define MI_POOLING_UNSPECIFIED (-1)
#define MI_POOLING_NONE 0
#define MI_POOLING_MEAN 1
#define MI_POOLING_CLS 2
#define MI_POOLING_LAST 3
#define MI_POOLING_RANK 4
/* The model's {arch}.pooling_type key (read for every architecture), or -1 when the GGUF has none
 * or the model is NULL. */
int32_t mi_model_pooling_type(const mi_model* model);
/* llama_model / hparams.causal_attn: 1 for llama and gpt2 (a causal decoder with a KV cache), 0 for
 * bert (a bidirectional encoder), -1 for NULL. */
int32_t mi_model_causal_attn(const mi_model* model);
/* llama_set_embeddings + pooling_type (InstanceEmbedding.cpp:24-32).  on != 0: every mi_decode from
 * the next one ends in the embedding rows and runs no output head -- mi_logits then returns NULL and
 * mi_topk / mi_gather / mi_gather_rows < 0, mi_last_error() saying that the context is in
 * embeddings mode; the KV cache is written as usual.  pooling MI_POOLING_UNSPECIFIED resolves to the
 * model's key, else NONE.  With a pooled type a call yields one row whatever its out_mode and takes
 * at most n_batch tokens.  on == 0: back to logits (pooling is still validated and kept).
 * Synchronises; leaves the KV cache alone; embeddings are not part of mi_state_get / mi_state_set.
 * 0 ok; < 0: null context, pooling outside -1..3, RANK. */
int32_t mi_ctx_set_embeddings(mi_ctx* ctx, int32_t on, int32_t pooling);
/* llama_pooling_type(ctx) (InstanceEmbedding.cpp:114): the resolved type; -1 for a null context. */
int32_t mi_ctx_pooling(const mi_ctx* ctx);
/* llama_get_embeddings_ith (pooling NONE; InstanceEmbedding.cpp:149) / llama_get_embeddings_seq
 * (pooled; InstanceEmbedding.cpp:154): n_embd floats, context-owned, valid until the next decode or
 * mi_embeddings call.  Synchronises.  NONE: rows as for mi_logits (-1 the last token's; 0..n-1
 * after MI_OUT_ALL, row 0 only after MI_OUT_LAST); pooled: row 0 or -1 is the sequence embedding.
 * NULL with a message when the mode is off, no decode has happened since it was set, or the row is
 * out of range. */
const float* mi_embeddings(mi_ctx* ctx, int32_t row);

/* ---- measurement: HIP events on the context's stream bracketing the FFN
 * gate/up GEMV launch of `layer` in every output-producing decode step (the
 * step's graph is split in three around it); layer < 0 disables.
 * mi_prof_read returns 1 and that launch's duration (microseconds) once per
 * timed step, 0 if no step was timed since the last read. ---- */
int32_t mi_prof_enable(mi_ctx* ctx, int32_t layer);
int32_t mi_prof_read(mi_ctx* ctx, float* us, int32_t n);
/* Algorithmic HBM bytes of one FFN gate/up launch (weights + activation in/out). */
int64_t mi_prof_ffn_bytes(const mi_ctx* ctx);
/* Algorithmic HBM bytes of the launch mi_prof_read last timed (the FFN gate/up launch). */
int64_t mi_prof_bytes(const mi_ctx* ctx);
/* Diagnostics: the form the context's decode steps take: 1 the streaming GEMV
 * launches (dgemv.hip; MoE: the attention half, the experts on gemv_kernel), 0 the gemv_kernel graph
 * (GPT-2), 2 an encoder context (bert: no decode step, one stateless pass per call on the kernels
 * of enc.hip), 3 an unquantised F16 LLaMA model (the F16 streaming GEMV launches of fgemv.hip; prompt
 * batches on the F16 MFMA GEMM of enc.hip); -1 for a null context. */
int32_t mi_decode_path(const mi_ctx* ctx);
/* Diagnostics: the form the most recent mi_decode call took (of a call of several physical batches:
 * its first): 0 one decode step per token, 1 the v_dot4 GEMM, 2 the tiled int8-MFMA GEMM, 3 the
 * short split-K GEMM, 4 the F16 MFMA GEMM, 5 an encoder pass; -1 for a null context or before the
 * first call.  Pure reporting. */
int32_t mi_batch_path(const mi_ctx* ctx);
/* Diagnostics: copies the per-workgroup s_memrealtime stamps (100 MHz) of the
 * first n_launch launches of the last decode step, [launch][512][8] uint64, to
 * out.  Returns the number of launches copied; 0 unless the library is the
 * diagnostic build (libmi_engine_stamps.so, compiled with -DMI_STAMPS). */
int32_t mi_debug_stamps(mi_ctx* ctx, uint64_t* out, int32_t n_launch);
/* Diagnostics: who quantises h for the FFN down launch of the streaming dense decode step, in every
 * layer from the next step on: 0 a dv_quant launch before it, 1 every down workgroup of 8 waves,
 * 2 every down workgroup of 16 waves and 16 rows.  The three compute the same bits; the context's
 * own choice is by measured speed.  0 ok, < 0 error (no such step, or no kernel for the form). */
int32_t mi_debug_down_quant(mi_ctx* ctx, int32_t form);

/* ---- op-level entry points (host buffers in/out) used by the parity tests ----
 * raw_blocks: GGUF-layout blocks of a rows x K matrix of ggml type `type`. */
int32_t mi_op_gemv(int32_t device, int32_t type, const void* raw_blocks, int32_t rows, int32_t K,
                   const float* x, float* y);
int32_t mi_op_dequant(int32_t device, int32_t type, const void* raw_blocks, int32_t rows, int32_t K,
                      float* out);
int32_t mi_op_quantize_q8_K(int32_t device, const float* x, int32_t K, int8_t* qs, float* d,
                            int32_t* bsums);
int32_t mi_op_topk(int32_t device, const float* logits, int32_t n, int32_t k, int32_t* ids, float* vals);
/* One decode step's attention (KQ -> soft_max -> KQV, Session.cpp:388's llama_decode inner
 * graph, flash_attn=false) of n_head f32 query heads over n_cells cells of an f16 K/V cache
 * [n_cells][n_head_kv*head_dim]; cells whose cell_pos > pos are masked.  out: [n_head*head_dim]. */
int32_t mi_op_attention(int32_t device, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_cells,
                        const float* q, const uint16_t* k_f16, const uint16_t* v_f16, const int32_t* cell_pos,
                        int32_t pos, float* out);
/* Which cache-attention kernel a launch of this head geometry would run (no device is touched).
 * mode: 0 a decode step within 512 cells that also quantises its output, 1 one that does not,
 * 2 a decode step past 512 cells (long_ok: the single launch may be used), 3 / 4 a short batch of
 * ntok tokens with / without the quantised output.  out[10]: kernel (0 none, 1 decode, 2 fused,
 * 3 long, 4 scores + pv), R, LPC, HG, NWV, grid_x, grid_y, block, dynamic LDS bytes, qsplit. */
int32_t mi_op_attn_plan(int32_t mode, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_ctx,
                        int32_t ntok, int32_t long_ok, int32_t* out);
/* Which int8-MFMA batch GEMM kernel a launch of this shape would run (no device is touched).
 * form: 0 the tiled GEMM of a physical batch, 1 the short streaming GEMM (npad 32 or 64; grouped: the
 * padded MoE rows).  type: the matrices' quant type; pair: a gate/up pair; rows[nseg]: the rows of
 * each matrix of the launch; grp_n > 0: a grouped (MoE) launch over grp_n experts of at most grp_max
 * rows each; ksplit, pre, gx (tiled): split-K parts, a pre-epilogue term, a bias or GELU epilogue;
 * n_cu (tiled): the device's compute units.  out[16]: kernel (0 none, 1 tiled, 2 short, 3 short
 * one-wave, 4 short one-wave lean), operand type, pair, pre, gx, grouped, stages (tiled), token
 * tiles (short), row blocks (short: row tiles), token blocks, K-parts (short), grid_x, grid_y,
 * grid_z, block, dynamic LDS bytes.  With kernel 0, mi_last_error() holds the launcher's message. */
int32_t mi_op_mmq_plan(int32_t form, int32_t type, int32_t pair, const int32_t* rows, int32_t nseg, int32_t npad,
                       int32_t K, int32_t grp_n, int32_t grp_max, int32_t ksplit, int32_t pre, int32_t gx, int32_t n_cu,
                       int32_t* out);
/* One decode step's attention as the engine launches it in `mode` (mi_op_attn_plan's 0, 1 or 2),
 * with the activation it publishes for the W_o launch.  The cache holds n_ctx rows
 * [n_ctx][n_head_kv*head_dim], of which cells 0 .. cell are the context (rows past `cell` are never
 * read into the result); a cell c is visible iff c <= cell and cell_pos[c] <= pos.
 * mode 0 (cell < 512): the launch also quantises its output, fmt bit 0 Q8_K, bit 1 Q8_0 (one or
 * both); the f32 row is returned only with want_f32 (the decode kernel stores it on request).
 * mode 1 (cell < 512): no quantised output (fmt 0).  mode 2 (cell >= 512): the scores and pv
 * launches, never the single exchange launch; their partials combined to f32 and, with fmt, also
 * quantised by the combine-and-quantise launch.
 * out: [n_head*head_dim] (K).  The activation unpacked from its published layout: q8k[K],
 * bsums[K/256][16] (16-element sums), dk[K/256]; q80[K], d0[K/32].  Buffers of a format not asked for
 * may be NULL.  Returns the plan's kernel (mi_op_attn_plan's out[0]), or -1: a geometry without a
 * plan in this mode is an error, nothing is launched. */
int32_t mi_op_attention_decode(int32_t device, int32_t mode, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                               int32_t n_ctx, int32_t cell, int32_t pos, const float* q, const uint16_t* k_f16,
                               const uint16_t* v_f16, const int32_t* cell_pos, int32_t fmt, int32_t want_f32,
                               float* out, int8_t* q8k, int32_t* bsums, float* dk, int8_t* q80, float* d0);
/* A short batch's attention (1 <= ntok <= 64 tokens, every token cell < 512), one grid row per token:
 * mi_op_attention_batch's inputs on the decode step's kernels.  quant 0: f32 rows only; 1 / 2: every
 * token's row also quantised to Q8_K / Q8_0 in the batch GEMMs' activation format, returned in token
 * order: q_out[ntok][K], d_out[ntok][K/256] (Q8_K) or [ntok][K/32] (Q8_0), and for Q8_K
 * bsums_out[ntok][K/256][8], the 32-element sums.  out: [ntok][K], K = n_head*head_dim.  Returns the
 * plan's kernel, or -1 (no plan for the geometry: nothing is launched). */
int32_t mi_op_attention_short(int32_t device, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_cells,
                              int32_t ntok, const float* q, const uint16_t* k_f16, const uint16_t* v_f16,
                              const int32_t* cell_pos, const int32_t* tok_cell, const int32_t* tok_pos,
                              int32_t quant, float* out, int8_t* q_out, float* d_out, int32_t* bsums_out);
/* The prompt-batch GEMM (Session.cpp:381-392's n_ubatch physical batches; ntok <= MI_MMQS_MAX,
 * default 64: the short-batch GEMM mmqs, otherwise the tiled int8-MFMA GEMM mmq32) of
 * ntok <= 512 token rows x[ntok][K] against a rows x K Q4_K / Q5_K / Q6_K / Q8_0 matrix: each row's
 * activation is quantised to Q8_K (Q8_0 for Q8_0 weights) as the CPU graph does, then
 * y[t][r] = vec_dot(W_r, q(x_t)).  With raw_up non-NULL the launch is the FFN gate/up pair
 * (raw_blocks = gate): y[t][r] = silu(gate_r . q(x_t)) * (up_r . q(x_t)).  y: [ntok][rows]. */
int32_t mi_op_gemm(int32_t device, int32_t type, const void* raw_blocks, const void* raw_up, int32_t rows,
                   int32_t K, int32_t ntok, const float* x, float* y);
/* A GPT-2 prompt-batch projection (llm_build_gpt2) on the tiled int8-MFMA GEMM, whatever ntok:
 * ntok <= 512 rows x[ntok][K] quantised by the batch path's quantiser -- norm_w and norm_b given:
 * layer_norm(x, eps) * norm_w + norm_b first (ggml_norm: sums in double, mean and variance in
 * float); both NULL: x itself -- then y[t][r] = vec_dot(W_r, q(x_t)) + bias[r] (bias NULL: none)
 * through the epilogue: 0 store, 1 + resid[t][r] (after the bias), 2 gelu(.) by ggml's f16 table.
 * y, resid: [ntok][rows].  q_out / d_out (nullable): the quantised activation in token order,
 * q_out[ntok][K] and d_out[ntok][K / 256] (Q8_K, k-quant matrices) or [ntok][K / 32] (Q8_0). */
int32_t mi_op_gemm_bias(int32_t device, int32_t type, const void* raw_blocks, int32_t rows, int32_t K,
                        int32_t ntok, const float* x, const float* norm_w, const float* norm_b, float eps,
                        const float* bias, const float* resid, int32_t epilogue, float* y, int8_t* q_out,
                        float* d_out);
/* The prompt-batch attention (attn_mfma: f16 MFMA) of ntok query tokens q[ntok][n_head*head_dim]
 * over an f16 cache of n_cells cells: token t sits in cell tok_cell[t] at position tok_pos[t] and
 * sees the cells c <= tok_cell[t] whose cell_pos[c] <= tok_pos[t] (llm_build_llama's kq_mask).
 * tok_cell must be ascending.  out: [ntok][n_head*head_dim]. */
int32_t mi_op_attention_batch(int32_t device, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                              int32_t n_cells, int32_t ntok, const float* q, const uint16_t* k_f16,
                              const uint16_t* v_f16, const int32_t* cell_pos, const int32_t* tok_cell,
                              const int32_t* tok_pos, float* out);
/* The decode step's streaming GEMV (dgemv.hip), one launch: x quantised on the device (Q8_K /
 * Q8_0 as the matrices need), then role 0 Q/K/V rows without RoPE (a second matrix of another type
 * = a second segment; y = [A x | B x]), 1 y = A x + resid, 2 y = silu(A x) * (B x) (gate/up pair),
 * 3 y = A x, 4 as 1 with x quantised inside the launch by every workgroup (the FFN down launch
 * of small models), 5 as 4 in 16-wave workgroups of 16 rows.  type2/raw2/rows2: the second matrix (raw2 NULL: none). */
int32_t mi_op_dgemv(int32_t device, int32_t role, int32_t type, const void* raw_blocks, int32_t rows, int32_t K,
                    int32_t type2, const void* raw_blocks2, int32_t rows2, const float* x, const float* resid, float* y);
/* The F16 decode step's streaming GEMV (fgemv.hip), one launch over F16 matrices [rows][K] (K a
 * multiple of 32, 32 .. 16384): y[r] = sum_k f16(x[k]) * W[r][k] in f32, then the role's epilogue --
 * 0 Q/K/V rows without RoPE, every row a Q row (a second matrix = further rows; y = [A x | B x],
 * both row counts even), 1 y = A x + resid, 2 y = silu(A x) * (B x) (gate/up pair, rows2 == rows),
 * 3 y = A x.  w2_f16 NULL: no second matrix. */
int32_t mi_op_fgemv(int32_t device, int32_t role, const uint16_t* w_f16, int32_t rows, int32_t K,
                    const uint16_t* w2_f16, int32_t rows2, const float* x, const float* resid, float* y);
/* Median microseconds of one fgemv launch of `role` over rows x K F16 matrices (role 2: a gate/up
 * pair of rows each), timed at the kernel's own start and end over `iters` launches after a warm-up,
 * each reading another copy of the weights (HBM, not the Infinity Cache).  bytes (nullable): the
 * matrix bytes one launch reads.  rows even. */
int32_t mi_op_fgemv_bench(int32_t device, int32_t role, int32_t rows, int32_t K, int32_t iters, float* median_us,
                          int64_t* bytes);
/* ---- the mixture-of-experts kernels, one at a time (build_moe_ffn: softmax gating, top-2) ----
 * The router of ntok token rows x[t * x_stride] (n_embd floats each, x_stride >= n_embd, a
 * multiple of 4): rms_norm(x, eps) * norm_w, logits against w [n_expert][n_embd] (F32), softmax,
 * the top 2 (ties: the lower index first) and their weights normalised over the two.  part
 * (nullable): the split-K halves [2][ntok][n_embd] of the projection that produced x, added first
 * and written back, x = (p0 + p1) + x.  sel_out / selw_out: [ntok][2]; x_out (nullable): the
 * [ntok][x_stride] rows after the call.  n_expert <= 64, n_embd a multiple of 256, <= 4096. */
int32_t mi_op_router(int32_t device, int32_t n_embd, int32_t n_expert, int32_t ntok, const float* x, int32_t x_stride,
                     const float* norm_w, float eps, const float* w, const float* part, int32_t* sel_out,
                     float* selw_out, float* x_out);
/* The grouping of n picks (sel[t * U + k] = expert of token t's slot k) by expert, E <= 16:
 * grp_out[2E + 1] = {off[0..E], cnt[0..E-1]} with off[e + 1] = off[e] + cnt[e] rounded up to 32;
 * rows_out[rows_cap] = the source token of each row (-1: padding), tokens ascending within an
 * expert; rowsel_out[rows_cap] = r or -1; pos_out[n] = the row of each pick.  rows_cap: the
 * capacity of rows_out / rowsel_out, at least (n + 31 E + 31) / 32 * 32 (the engine's value).
 * Every output is pre-filled with 0x80808080, so an entry the kernel did not write shows. */
int32_t mi_op_moe_group(int32_t device, const int32_t* sel, int32_t n, int32_t U, int32_t E, int32_t rows_cap,
                        int32_t* grp_out, int32_t* rows_out, int32_t* rowsel_out, int32_t* pos_out);
/* The experts' grouped GEMM of a prompt batch: raw_blocks (and raw_up) hold n_expert matrices of
 * rows x K back to back; sel[ntok][2] are each token's two distinct experts.  The picks are grouped
 * (mi_op_moe_group's kernel), their rows quantised to Q8_K / Q8_0 -- per_pick 0: x is [ntok][K],
 * pick i reads token i / 2's row (the gate/up stage); per_pick 1: x is [2 ntok][K], one row per
 * pick (the down stage) -- and multiplied by their experts' matrices: mode 0 the tiled grouped GEMM
 * (any type of mi_op_gemm, ntok <= 512), mode 1 the short grouped GEMM (Q4_K / Q5_K / Q6_K,
 * ntok <= 64) with its K-parts added.  raw_up non-NULL: the gate/up pair, silu(gate) * up.
 * y[2 ntok][rows]: row i = pick i (token i / 2 through expert sel[i]). */
int32_t mi_op_moe_gemm(int32_t device, int32_t mode, int32_t type, const void* raw_blocks, const void* raw_up,
                       int32_t n_expert, int32_t rows, int32_t K, int32_t ntok, const float* x, int32_t per_pick,
                       const int32_t* sel, float* y);
/* The decode step's two expert launches after the router, with the router's result given:
 * h_out[k] = silu(gate[sel[k]] c) * (up[sel[k]] c), c = rms_norm(x, eps) * norm_w (k = 0, 1), then
 * x_out = ((down[sel[0]] h0) * selw[0] + (down[sel[1]] h1) * selw[1]) + x [+ addend].  gate / up:
 * n_expert matrices of n_ff x n_embd back to back, down: of n_embd x n_ff; addend (nullable):
 * [n_embd].  h_out: [2][n_ff], x_out: [n_embd]. */
int32_t mi_op_moe_decode(int32_t device, int32_t type, const void* gate, const void* up, const void* down,
                         int32_t n_expert, int32_t n_embd, int32_t n_ff, const float* x, const float* norm_w, float eps,
                         const int32_t* sel, const float* selw, const float* addend, float* h_out, float* x_out);
/* The encoder pass's dense F16 GEMM (enc.hip, v_mfma_f32_32x32x16_f16): y[t][r] = sum_k f16(x[t][k]) *
 * w[r][k] in f32, then the epilogue -- 0 none, 1 + bias[r], 2 gelu(. + bias[r]) by ggml's f16 table,
 * 3 (. + bias[r]) + resid[t][r].  w: [rows][K] f16 bits, x: [ntok][K], resid / y: [ntok][rows];
 * rows % 32 == 0, K % 32 == 0, 1 <= ntok <= 512. */
int32_t mi_op_gemm_f16(int32_t device, const uint16_t* w_f16, int32_t rows, int32_t K, int32_t ntok,
                       const float* x, const float* bias, const float* resid, int32_t epilogue, float* y);
/* The encoder pass's bidirectional attention (enc.hip): every token over all ntok <= 512 tokens, no
 * mask, scale 1 / sqrtf(head_dim); q / out: f32 [ntok][n_head * head_dim], k / v: f16 bits of the same
 * shape; head_dim 32 or 64. */
int32_t mi_op_attention_enc(int32_t device, int32_t n_head, int32_t head_dim, int32_t ntok,
                            const float* q, const uint16_t* k_f16, const uint16_t* v_f16, float* out);
/* Median device time (us) of `iters` launches of mi_op_gemv's GEMV (micro-benchmark). */
int32_t mi_op_gemv_bench(int32_t device, int32_t type, const void* raw_blocks, int32_t rows, int32_t K,
                         int32_t iters, float* median_us);

#ifdef __cplusplus
}
#endif
#endif /* MI_ENGINE_H */
