/* librdx -- C ABI of the MI355X-native RaDialog inference path (image encode -> prompt project -> Llama greedy decode).
 *
 * The reference (ChantalMP/RaDialog) has no FFI: its boundary for this path is the Python object API that demo.py /
 * test.py call. librdx sits directly underneath radialog_amd's mirror of that API; each entry point below names the
 * reference interface it replaces. Conventions:
 *   - extern "C", plain pointers and sizes, no torch types. Every data pointer is a DEVICE pointer on the context's
 *     GPU (what torch.Tensor.data_ptr() returns) unless the name ends in _host.
 *   - every function returns 0 on success or a negative error code; rdx_last_error() returns the message. Nothing
 *     throws across the boundary; the library never frees caller memory; outputs are written to caller buffers.
 *   - one rdx_ctx per (process, device); not thread-safe (callers serialise per context). All work is enqueued on
 *     the context's own HIP stream; rdx_sync() blocks until it has drained. Functions that return host-visible
 *     results (rdx_generate's n_steps) synchronise internally.
 */
#ifndef RDX_H
#define RDX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rdx_ctx rdx_ctx;

enum { RDX_DTYPE_F16 = 0, RDX_DTYPE_BF16 = 1 };
enum { RDX_W_GEMM = 0,   /* [rows=N][cols=K] fp32 -> model dtype, re-laid-out into MFMA fragment order            */
       RDX_W_TENSOR = 1, /* [rows][cols] fp32 -> model dtype, row-major (embeddings, norm weights, LoRA B, RoPE)    */
       RDX_W_F32 = 2,    /* [rows][cols] fp32 kept as fp32 (biases, LayerNorm gamma/beta)                           */
       RDX_W_GEMM_FP8 = 3, /* quantised to OCP e4m3 with one absmax/448 scale per output row and stored ONLY in that
                            * form (64-deep MFMA fragment order): prefill and batch >= 3 decode multiply fp8 x fp8
                            * (activations e4m3 with a scale per row and K group), batch <= 2 expands the bytes in
                            * registers; a shape without an fp8 kernel makes the call return -8, there is no
                            * dequantised copy to fall back to (BASELINE configs[4]). The 2r LoRA-A rows ride the QKV weight
                            * and are therefore e4m3 too (own row scales, e4m3 input); only LoRA-B is a model-dtype epilogue */
       RDX_W_GEMM_W4 = 4 };  /* int4 group-quantised (W4A16; the format: radialog_amd/w4.py): groups of 128 k of one row, symmetric,
                            * s = T(absmax / 7), q = clamp(rint(w / s), -8, 7). int4 is a STORAGE format of the batch <= 2 step's weight
                            * stream, not an arithmetic: the weight IS its dequantised value W' = T(q s). The library keeps a fragment-packed
                            * model-dtype copy of W', which prefill, batch >= 3, scoring, beam search and the append calls multiply with the
                            * kernels of RDX_W_GEMM, and for gate/up, down_proj and QKV the int4 stream (4.125 bits per weight), which the
                            * batch <= 2 step decodes to exactly W' in registers: the same bits as a RDX_W_GEMM context loaded with W'. Rows
                            * of "l<i>.wqkv" from 3 * hidden on (the 2r LoRA-A rows) are NOT quantised (W' = T(W)); their tiles stream raw.
                            * o_proj is quantised as a model weight but still streams its packed W' bytes inside the fused attention
                            * launch, and the lm_head is meant to stay RDX_W_GEMM. Returns -8 with a message in an f16 context (not built),
                            * for K % 128 != 0 and in a context that also holds RDX_W_GEMM_FP8 weights; -1 for an Inf / NaN weight. Not
                            * built: batch >= 3 / prefill int4 kernels, pre-quantised GPTQ / AWQ tensors, zero points. */

typedef struct rdx_config {
    int dtype;                                     /* RDX_DTYPE_* : arithmetic type of weights/activations         */
    /* Llama decoder (modeling_llama_imgemb.py:433-843; dims of lmsys/vicuna-7b-v1.3) */
    int vocab, hidden, inter, layers, heads, max_pos;
    float rms_eps;
    int lora_r; float lora_scale;                  /* 0 = no adapter; peft LoRA on q_proj,v_proj (finetune.py:167) */
    int qformer_dim;                               /* img_proj_layer input width (demo.py:229)                     */
    /* Q-Former (Qformer.py; blip2.py:47-62) */
    int q_hidden, q_layers, q_heads, q_inter, q_enc_width, q_nquery, q_cross_freq;
    float q_ln_eps;
    /* BioViL-T image encoder (biovil_t/encoder.py:86-136, resnet.py:15-47, model.py:33-91) */
    int v_img, v_stem, v_planes[4], v_blocks[4], v_b2v, v_proj;
    float v_ln_eps;
    /* capacities */
    int max_batch;                                 /* decode rows held in the KV cache: 1 .. 128 (round 5: rows 33-128 decode in 32-row blocks that
                                                    * share an XCD's L2 -- model dtype, or the fp8 x fp8 kernels with fp8 weights, RDX_W_GEMM_FP8)    */
    int max_len;                                   /* KV slots per row (prompt + generated), multiple of 32        */
    int enable_vision, enable_llama;               /* build only one half if 0                                     */
    /* findings classifier (findings_classifier/chexpert_model.py:7-21): the same trunk + projector (v_*) followed by
     * avg_pool2d(cls_pool), fc1 -> ReLU -> fc2. A classifier context sets enable_cls = 1 and enable_vision = 0.    */
    int enable_cls, cls_hidden, cls_classes, cls_pool;
} rdx_config;

/* lifecycle -- replaces model construction (demo.py:149-153 init_blip, :221-236 init_vicuna) */
int rdx_create(rdx_ctx** out, int device_id, const rdx_config* cfg);
void rdx_destroy(rdx_ctx* ctx);
/* 16 hex digits: radialog_amd/build.py source_hash() over the kernel / ABI sources this binary was compiled from ("unstamped" when built
 * without the build script). The Python loader compares it with the hash of the sources next to it and refuses a mismatch. */
const char* rdx_build_hash(void);
const char* rdx_last_error(rdx_ctx* ctx);          /* ctx may be NULL: last error of a failed rdx_create           */
int rdx_sync(rdx_ctx* ctx);
void* rdx_stream(rdx_ctx* ctx);                    /* hipStream_t of the context                                   */

/* weights -- replaces load_checkpoint / from_pretrained / PeftModel.from_pretrained (base_model.py:29-56,
 * demo.py:224-234). `name` is an engine tensor name (radialog_amd/weights.py maps reference state_dict keys to them);
 * `data` is a device fp32 tensor, copied/converted into library-owned storage (the caller may free it afterwards). */
int rdx_set_weight(rdx_ctx* ctx, const char* name, const float* data, int64_t rows, int64_t cols, int kind);
/* The same from a source tensor of another element type: src_dtype RDX_SRC_F32 / RDX_SRC_F16 / RDX_SRC_BF16 (`data` is then a device
 * tensor of that type). A real Vicuna-7B checkpoint is stored in fp16 (from_pretrained(torch_dtype=float16), demo.py:224-226): its
 * tensors go to the library as they are instead of being inflated to fp32 on the host first. fp16 / bf16 sources are widened
 * exactly; the result is bit-identical to rdx_set_weight on the widened tensor. */
enum { RDX_SRC_F32 = 0, RDX_SRC_F16 = 1, RDX_SRC_BF16 = 2 };
int rdx_set_weight_typed(rdx_ctx* ctx, const char* name, const void* data, int src_dtype, int64_t rows, int64_t cols, int kind);
int rdx_finalize_weights(rdx_ctx* ctx);            /* resolves names, checks completeness, allocates workspaces    */

/* image transform -- replaces create_chest_xray_transform_for_inference(resize, center_crop_size)(pil_image) (model/lavis/data/ReportDataset.py:96-106;
 * demo.py:144 / :251: 512 -> 448 for the report model, demo.py:169: 512 -> 488 for the findings classifier) = torchvision Resize(resize) -> CenterCrop(crop)
 * -> ToTensor -> ExpandChannels on the 8-bit "L" image of demo.py:205-218. img: DEVICE uint8 [H][W] row-major; out: DEVICE float32 [3][crop][crop] in [0, 1].
 * Resize on a PIL image is PIL.Image.resize(BILINEAR) (Pillow Resample.c: antialiased triangle filter, two fixed-point passes, uint8 in between): the output
 * equals Pillow's bit for bit. Works on any context (no weights involved). Error: the resized image is smaller than the crop (torchvision would zero-pad). */
int rdx_transform_image(rdx_ctx* ctx, const uint8_t* img, int H, int W, int resize, int crop, float* out);

/* Blip2Qformer.forward_image (blip2_qformer.py:467-484): image float32[B,3,S,S] ->
 *   qformer_out float32[B,n_query,q_hidden] (last_hidden_state), image_embeds float32[B,P,v_proj] (nullable). */
int rdx_encode_image(rdx_ctx* ctx, const float* image, int batch, float* qformer_out, float* image_embeds);
/* Same with a prior study: MultiImageEncoder.forward(current_image, previous_image) (biovil_t/encoder.py:117-123) runs
 * both images through the trunk and takes the difference features from the VisionTransformerPooler
 * (biovil_t/transformer.py:73-224). No RaDialog caller passes a previous image; optional mode of the encoder. */
int rdx_encode_image2(rdx_ctx* ctx, const float* image, const float* previous_image, int batch, float* qformer_out,
                      float* image_embeds);

/* ChexpertClassifier.forward (findings_classifier/chexpert_model.py:15-21; call site demo.py:155-170,:256-261):
 * image float32[B,3,S,S] (S = v_img, 488 in demo.py) -> logits float32[B,cls_classes]; the caller applies sigmoid > 0.5. */
int rdx_classify_findings(rdx_ctx* ctx, const float* image, int batch, float* logits);

/* LlamaForCausalLM.generate(..., num_beams=1) as the reference calls it (demo.py:290-297, test.py:339-348):
 * greedy search (transformers 4.28.1 GenerationMixin.greedy_search) over LlamaForCausalLM.forward with the image
 * splice (modeling_llama_imgemb.py:571-594).
 *   ids          int32[B,T]   left-padded prompt token ids
 *   mask         int32[B,T]   attention mask, or NULL -> ids != pad_id (HF's inferred mask)
 *   qformer_embs float32[B,32,qformer_dim] or NULL (no image splice: `dicom is None and not use_img`)
 *   eos_id       -1 = never stop (throughput runs)
 *   out_tokens   int32[B,max_new]  generated ids; finished rows emit pad_id
 *   scores       model-dtype [max_new][B][vocab] per-step logits (`output_scores=True`), or NULL
 *   n_steps_host host int: number of steps executed (< max_new when every row hit EOS)
 *   use_graph    replay one captured hipGraph per decode step instead of ~160 eager launches */
int rdx_generate(rdx_ctx* ctx, const int32_t* ids, const int32_t* mask, int batch, int T, const float* qformer_embs,
                 int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* scores, int* n_steps_host,
                 int use_graph);

/* The two halves of rdx_generate, for callers that drive the loop themselves (prepare_inputs_for_generation +
 * forward, modeling_llama_imgemb.py:705-836). rdx_prefill runs the prompt and selects token 0; each rdx_decode_step
 * consumes the previously selected token and selects the next. logits: model-dtype [B][vocab] of that step or NULL. */
int rdx_prefill(rdx_ctx* ctx, const int32_t* ids, const int32_t* mask, int batch, int T, const float* qformer_embs,
                int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* logits);
int rdx_decode_step(rdx_ctx* ctx, void* logits);
/* The same step on caller-supplied input ids int32[B] (device) instead of the token the previous step selected: the loop-driving
 * caller's forward(input_ids=[B,1], past_key_values) (modeling_llama_imgemb.py:705-836) -- teacher forcing, constrained decoding. */
int rdx_decode_step_ids(rdx_ctx* ctx, const int32_t* ids, void* logits);

/* Logits rules of the greedy search: transformers 4.28.1 `_get_logits_processor` as generate(repetition_penalty=, no_repeat_ngram_size=,
 * min_new_tokens=) builds it, applied in that order to every step's logits row x (model dtype) before the argmax. The history of a row is what HF
 * holds in input_ids: the prompt as passed (left pads and <IMG> ids included), then every token selected so far (the pad_id of a finished row too).
 *   repetition_penalty p > 0 (1.0 = off): every DISTINCT token t of the history, once: x[t] = T(x[t] < 0 ? x[t] * p : x[t] / p), fp32 arithmetic with
 *                an IEEE division, one round-to-nearest-even to the model dtype -- torch.where(score < 0, score * p, score / p), bit for bit
 *   no_repeat_ngram_size n >= 0 (0 = off): with history length L >= n - 1, every j with hist[j .. j+n-2] == hist[L-n+1 .. L-1] and j + n - 1 < L
 *                sets x[hist[j+n-1]] = -inf
 *   min_new_tokens m >= 0 (0 = off): while the row has generated fewer than m tokens and eos_id >= 0, x[eos_id] = -inf
 * The processed row is what `logits` / `scores` receive (HF's .scores), the token is its argmax (lowest index on ties), then the greedy rule as before.
 * rdx_set_logits_rules sets the rules of the NEXT rdx_prefill / rdx_generate / rdx_decode_step* calls on this context; NULL or all-neutral
 * (1.0, 0, 0) = off: launches, graph and outputs are exactly those of a context that never heard of rules. Returns -1 for p <= 0 or not finite,
 * n < 0, m < 0. With rules on, rdx_decode_step_ids records the caller's ids in the history (not the token it replaced), and rdx_beam_search,
 * rdx_prefill_append and rdx_generate_append return -1: beam search applies processors to log-softmax scores and reorders histories, append needs
 * the history carried across calls. */
typedef struct rdx_logits_rules { float repetition_penalty; int no_repeat_ngram_size; int min_new_tokens; } rdx_logits_rules;
int rdx_set_logits_rules(rdx_ctx* ctx, const rdx_logits_rules* rules);

/* Sampled decoding: transformers 4.28.1 `sample` as generate(do_sample=True, temperature=, top_k=, top_p=) runs it -- processors, then warpers, then
 * the draw -- inside the decode step, in the place of the argmax. Row b at draw index n (= the number of tokens the row has generated so far: 0 for the
 * token the prefill selects):
 *   1. the logits rules above, exactly as without sampling, give x (model dtype T)
 *   2. temperature t, finite, > 0 (1.0 = off): s_i = T(float(x_i) / t), an fp32 IEEE division and one round-to-nearest-even -- scores / temperature on a
 *      CPU tensor of the model dtype, the convention of the repetition penalty
 *   3. top_k k >= 0 (0 = off): v = the min(k, vocab)-th largest s; every s_i < v is dropped, ties with v stay (TopKLogitsWarper)
 *   4. top_p p in (0, 1] (1.0 = off): over the survivors w_i = exp(s_i - max s); for a value v, M(v) = sum of w_j over s_j <= v, divided by the sum of all
 *      w; element i is dropped iff M(s_i) <= 1 - p and s_i is not the maximum. This is TopPLogitsWarper(min_tokens_to_keep=1) stated on values
 *      instead of on a sort order; it differs from HF only inside a group of EQUAL values that straddles the boundary, where HF's result depends on
 *      the order an unstable sort leaves them in (here the whole group stays or goes)
 *   5. the processed row is what `logits` / `scores` receive, in place: kept elements hold s_i, dropped ones -inf (HF's .scores)
 *   6. the draw: u24 = philox4x32_10(counter = (b, n, 0, 0), key = (seed_lo, seed_hi))[0] >> 8. Masses are integers, q_i = rint(w_i * 2^32) as uint64
 *      (w_i in fp32 on the device); C = their inclusive prefix sum in index order over the kept elements; target = (u24 * C_last) >> 24; the token is
 *      the first i with C_i > target. Then the EOS / pad rule and the state advance of every step.
 * Integer masses make every sum independent of the order it is taken in: the same inputs, seed and draw index give the same token and the same scores
 * row on every run, eager or replayed from the step graph.
 * rdx_set_sampling sets the selection of the NEXT rdx_prefill / rdx_generate / rdx_decode_step* / rdx_prefill_append / rdx_generate_append calls; NULL or
 * do_sample == 0 = off: launches, graph and outputs are exactly those of a context that never sampled, with or without rules. Returns -1 for a t that
 * is not finite and > 0, k < 0, p outside (0, 1], weights not finalised, or a vocab whose row does not fit the kernel's LDS. It composes with
 * rdx_set_logits_rules (rules, then warpers, then the draw); the append calls work while the rules are off (sampling needs no history);
 * rdx_beam_search returns -1 while sampling is on (beam-sample is not built). Without a caller buffer the lm_head writes into the context's own rows.
 * The seed is read from device memory by the kernel: a new seed does not re-capture the step graph, a change of t / k / p or of do_sample does. */
typedef struct rdx_sampling { int do_sample; float temperature; int top_k; float top_p; uint64_t seed; } rdx_sampling;
int rdx_set_sampling(rdx_ctx* ctx, const rdx_sampling* s);

/* Generation log-probs: for every (row, step) of a conversation, how sure the selection was of the token the step wrote to out_tokens[row][step]. Opt-in; with
 * the option off every launch and every output bit is that of a context that never had it.
 * Let x be the step's scores row as the selection kernel left it, over columns 0 .. vocab - 1 only: the raw lm_head logits for plain greedy, the row processed
 * in place under rdx_set_logits_rules, the warped row under rdx_set_sampling -- what HF's .scores holds, so that `chosen` is what
 * compute_transition_scores(..., normalize_logits=True) computes. With m = max x, S = sum exp(float(x_i) - m), in fp32 and never rounded to the model dtype
 * (the formula of the scoring pass below):
 *   chosen              = (float(x_tok) - m) - log(S)
 *   top_ids[0 .. n)     the n columns with the largest x in descending order, lowest index on ties; the order is taken on the model-dtype values, which are
 *                       exact. -inf entries (banned or dropped columns) follow once the finite ones run out, with log-prob -inf. NaN columns never enter;
 *                       a slot without a candidate holds (-1, 0.0f)
 *   top_lp[0 .. n)      their log-probs by the same formula
 * One launch of logprob_step_k (csrc/logprob.hip), one workgroup per row, rides behind the selection launch of the prompt's token-0 call, of every
 * single-step call and of the captured step; every reduction runs in a fixed order that does not depend on where the row lies: the same row gives the same
 * bits with and without a scores buffer, eager or replayed. A step at or beyond max_new writes nothing. Entries of steps that have not run read
 * (0.0f, -1, 0.0f); a prefill resets the rows it starts. A row that has emitted EOS keeps getting entries, for the pad token the step's tail writes
 * (radialog_amd's Python layer masks everything behind a row's first EOS to (0.0, -1, 0.0)).
 * rdx_set_logprobs: top_n = -1 switches the option off, 0 .. RDX_MAX_TOP_LOGPROBS on (0: the chosen token only) for the NEXT prefill / generate / decode-step /
 * append calls; it is part of the step graph's key. Returns -1 with a message for a top_n outside that range, before rdx_finalize_weights, for a vocabulary
 * whose row does not fit the kernel's LDS (or above 65536 columns), and inside a row session ("rdx_rows_end first"). The first call allocates context-owned buffers (chosen
 * float [max_batch][max_len], top_ids int32 and top_lp float [max_batch][max_len][8]) whose addresses never change; without a caller buffer the lm_head writes
 * its rows into the context's own, as under rules. While the option is on, rdx_beam_search (beams return sequence scores) and rdx_rows_begin (a moved row's
 * entries would have to move with it) return -1 with a message naming "logprobs". fp8 / int4 / coded weights and the fp8 KV cache need nothing special.
 * rdx_get_logprobs drains the stream and copies the current conversation's entries to HOST memory: chosen_host float [batch][n_steps], top_ids_host int32 and
 * top_lp_host float [batch][n_steps][top_n] (both nullable). Returns -1 while the option is off or when batch / n_steps exceed the conversation's rows /
 * max_new.
 * Not built: row sessions, beams, log-probs of the raw logits while rules or warpers are on, the row's entropy. */
#define RDX_MAX_TOP_LOGPROBS 8
int rdx_set_logprobs(rdx_ctx* ctx, int top_n);
int rdx_get_logprobs(rdx_ctx* ctx, int batch, int n_steps, float* chosen_host, int32_t* top_ids_host, float* top_lp_host);

/* Scoring given tokens: LlamaForCausalLM.forward(input_ids, attention_mask, labels=) of the reference (modeling_llama_imgemb.py:705-793) -- the logits of
 * every position and what its shifted cross-entropy is made of -- from ONE pass over the prompt's kernels (no decode steps).
 *   ids / mask / qformer_embs  device pointers as for the prefill call: the left-padded prompt, the mask (NULL -> ids != 0), the image splice
 *   labels_host  HOST int32[B][T], HF's convention: the token at position t, or -100 for "not scored"
 *   logprob      float[B][T] (device): at t >= 1 with labels[b][t] != -100, log p(labels[b][t] | ids[b][:t]); 0 at every other entry and at t = 0
 *   top1         nullable int32[B][T] (device): at the same entries the model's argmax for position t (lowest index on ties); -1 elsewhere
 *   logits       nullable model dtype [B][T][vocab] (device): the logits of every position (forward().logits). NULL: only the rows whose successor is
 *                scored pass the lm_head, and the library never holds more than one chunk of logits
 * For a scored entry, with x the model-dtype logits row of position t - 1 over columns 0 .. vocab - 1 only (the lm_head's pad columns never enter):
 *   m = max x, S = sum exp(float(x_i) - m), logprob = (float(x_label) - m) - log(S) in fp32, not rounded to the model dtype (score_rows_k, score.hip).
 * Every reduction runs in a fixed order without floating-point atomics: the same inputs give the same bits on every run. The loss of the reference is
 * -(sum of the scored logprob entries) / (their number).
 * The rows pass the final RMSNorm and the lm_head in chunks of "score_chunk" rows (an option of the set-option call; 0 = all at once) through one
 * logits workspace [chunk][vocab padded to 16].
 * Returns -1, with a message and nothing written, for: a label outside [0, vocab) other than -100; T > max_len, T > max_position_embeddings or
 * batch > max_batch; weights not finalised; an fp8-weight context (an all-position lm_head would need a quantisation convention that the oracle
 * does not define below batch 3).
 * The call overwrites the KV cache and leaves the context without a conversation, as after creation: the decode-step and append calls return -1 until the
 * next prefill, and a token history of the logits rules is gone. Rules and sampling set on the context stay set and are ignored here: nothing is selected.
 * The call returns after the stream has drained. No scoring behind a kept prefix, none under beam search. */
int rdx_score(rdx_ctx* ctx, const int32_t* ids, const int32_t* mask, int batch, int T, const float* qformer_embs, const int32_t* labels_host,
              float* logprob, int32_t* top1, void* logits);

/* Multi-turn re-prompting (test.py:440-674, demo.py:277-305: the reference re-runs the whole conversation each turn). The
 * next turn's prompt usually starts with the previous prompt + answer; its KV rows are still in the cache. These calls keep the
 * first keep_len cache slots of every row (keep_len <= cached positions = previous T + tokens consumed; the caller compares
 * token ids: radialog_amd LlamaForCausalLM.generate does) and run only ids_tail int32[B,T_tail] (no padding, no <IMG>
 * splice) behind them: positions, causal mask and logits are those of the full sequence. Same outputs as rdx_prefill /
 * rdx_generate. */
int rdx_prefill_append(rdx_ctx* ctx, const int32_t* ids_tail, int batch, int T_tail, int keep_len, int max_new, int eos_id,
                       int pad_id, int32_t* out_tokens, void* logits);
int rdx_generate_append(rdx_ctx* ctx, const int32_t* ids_tail, int batch, int T_tail, int keep_len, int max_new, int eos_id,
                        int pad_id, int32_t* out_tokens, void* scores, int* n_steps_host, int use_graph);

/* Prompt-lookup decoding (transformers' generate(prompt_lookup_num_tokens=, max_matching_ngram_size=)): batch 1, greedy. Where the answer copies text that
 * already stands in the sequence (a corrected report, a quoted document), several tokens per weight stream are nearly free: propose the tokens that followed
 * the same n-gram earlier, run them through the decoder in ONE pass of the append path's <= 32-row kernels, keep the longest prefix the model agrees with.
 * Opt-in; with the option off no launch, no graph key and no output bit changes, and every other call ignores the option.
 * The draft rule. H = corpus | prompt ids as passed | every emitted token. For n = ngram_max down to ngram_min: among the starts j with H[j .. j+n) equal to
 * the last n tokens of H and j + n < len(H), the largest; the draft is H[j+n .. min(j+n+draft_len, len(H))). The first n with a match wins; no match, no
 * draft. A draft is clipped so that a pass never emits beyond max_new (d <= max_new - emitted - 1) and never writes a cache slot at or beyond T + max_new.
 * Every forward: d == 0 is the captured batch-1 step; d > 0 one verify pass over [last emitted token, draft_1 .. draft_d] at slots L .. L + d behind the L
 * kept ones (the layer loop of rdx_prefill_append), the final RMSNorm and the lm_head over the d + 1 rows. Row j's argmax (lowest index on ties, real
 * vocabulary columns only) is compared with draft_{j+1}: with a accepted drafts the pass emits draft_1 .. draft_a and argmax_a; an EOS among them ends the
 * emission and the call, pads follow. The next slot is L + a + 1; the rejected slots behind it are overwritten before anything reads them.
 * One launch of lookup_accept_k (csrc/lookup.hip) behind the lm_head of either kind of forward does all of that on the device; the host reads 8 bytes per
 * forward (the next d and the finished flag, the next slot) for its launch shapes: one small copy and one sync per forward.
 * The contract is NOT bit identity with rdx_generate: a pass runs the prompt kernels, a plain step the chained batch-1 kernels, and their logits differ in
 * rounding, which can flip a near-tie. What holds: (1) tokens[i] is the lowest-index argmax of scores[i], exactly; (2) scores[i] are the model's logits on the
 * call's own emitted prefix, within the project's parity bar; (3) given the emitted tokens, drafts and accepted counts follow the rule above exactly;
 * (4) a call in which no draft is ever found gives rdx_generate's tokens and scores bit for bit.
 *   rdx_set_lookup  draft_len in [1, 15], ngram_max in [1, 8], ngram_min in [1, ngram_max]; NULL or draft_len == 0 switches the option off.
 *   corpus       nullable HOST int32[n_corpus], n_corpus >= 0: extra token ids searched in front of the prompt (copied into a context-owned buffer)
 *   scores       nullable device buffer, model dtype [max_new][vocab]: for every emitted token the logits row it was chosen from
 *   n_tokens_host tokens emitted (EOS included); stats_host int[3] = {verify passes, tokens drafted, tokens accepted}
 *   trace_host   nullable int[trace_cap][2]: (drafted, accepted) of every forward behind the prompt in order; a plain step records (0, 0)
 * The call leaves an ordinary conversation of n_tokens steps behind: rdx_decode_step* and rdx_generate_append continue it.
 * Returns -1 with a message, the previous conversation untouched, for: the option off; batch != 1; logits rules, sampling or logprobs on; inside a row session;
 * the fp8 KV cache ("kv_fp8": the kept prefix is not held in the model dtype); an fp8-weight context (the all-row lm_head of a pass has no quantisation
 * convention below batch 3, as for rdx_score); T + max_new beyond max_len / max_position_embeddings. int4 and coded weights work: the plain steps stream
 * them, the passes multiply the packed W' / W, the same weights.
 * Not built: batch > 1, sampling (speculative sampling), logits rules, beams, row sessions, a draft model, a captured pass, a split-key verify attention. */
typedef struct rdx_lookup { int draft_len; int ngram_max; int ngram_min; } rdx_lookup;
int rdx_set_lookup(rdx_ctx* ctx, const rdx_lookup* lookup);
int rdx_generate_lookup(rdx_ctx* ctx, const int32_t* ids, const int32_t* mask, int batch, int T, const float* qformer_embs, const int32_t* corpus_host, int n_corpus,
                        int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* scores, int* n_tokens_host, int* stats_host, int* trace_host,
                        int trace_cap);

/* LlamaForCausalLM.generate(..., num_beams = k > 1) (test.py:467,:629 pass `num_beams=args.num_beams`): transformers 4.28.1
 * GenerationMixin.beam_search driven by BeamSearchScorer (length_penalty 1.0, early_stopping False, one returned hypothesis per
 * prompt by default) over the same forward, with `_reorder_cache` (modeling_llama_imgemb.py:838-843) between steps.
 *   ids / mask / qformer_embs  rows = groups * num_beams, ALREADY expanded the way _expand_inputs_for_generation lays them out
 *                (row r belongs to prompt r / num_beams; the k rows of a prompt are identical); rows <= max_batch
 *   out_tokens_host int32[groups][max_new] (HOST): generated ids of the best hypothesis, pad_id behind its end; the caller appends
 *                the EOS / pads to a common length like BeamSearchScorer.finalize. out_len_host[groups]: generated length;
 *                out_score_host[groups] (nullable): sum of log-probs / length ** length_penalty
 *   step_scores  nullable DEVICE buffer, model dtype [max_new][rows][vocab]: the processed next-token scores (log_softmax) of every
 *                step, what HF returns as `.scores` for beam search
 *   n_steps_host decoder forwards consumed (prompt included) */
int rdx_beam_search(rdx_ctx* ctx, const int32_t* ids, const int32_t* mask, int groups, int num_beams, int T, const float* qformer_embs,
                    int max_new, int eos_id, int pad_id, float length_penalty, int early_stopping, int32_t* out_tokens_host,
                    int32_t* out_len_host, float* out_score_host, void* step_scores, int* n_steps_host);

/* Row sessions: continuous batching. The decode step costs nearly the same with 4 live rows as with 32 (it is bound by weight traffic), so a batch that
 * waits for its longest report decodes pads in every row that finished early. In a session the step runs on `rows` LIVE rows and the caller refills a
 * finished row from its queue of waiting prompts while the neighbours go on decoding. No reference counterpart (HF generate has no such loop).
 * A refill runs R prompts through the prompt path -- the launches of rdx_prefill(batch = R, T) -- into `stage` STAGING rows above the live ones, then moves
 * each staged row (the KV of all layers, positions [0, ceil16(T)), and its decode state) into its target row; staging rows never take part in a step. A row
 * nobody uses is PARKED: cache slot 0, position 0, finished, step count = cap; it still runs a one-position step but writes no token, and every rdx_rows_step
 * call parks it again first, as it does a row whose end a poll has seen, so no number of steps carries such a row out of its cache row.
 * A request ends at EOS (the rule of every greedy step: then the row emits pad_id) or at its own cap, which the CALLER enforces from steps_host: tokens past a
 * request's own cap are to be ignored. The library keeps a host mirror of every row's cache slot and step count (T and 1 at the refill, + 1 per step).
 * Every call returns -1, with a message and nothing enqueued, for: any rdx_rows_* call but begin outside a session; begin inside one; inside a session
 * rdx_prefill*, rdx_generate*, rdx_decode_step*, rdx_score, rdx_beam_search and rdx_time ("rdx_rows_end first"), and switching rules or sampling on; begin
 * while logits rules or sampling are on (a moved row's token history and draw index would have to move with it: out of scope); the shape rules below.
 * All weight formats work (bf16 coded, int4, fp8, f16): only existing prompt and step launches run, plus the two copy kernels of rows.hip. */
/* Opens a session with every row parked and out_tokens (DEVICE int32[rows][cap], the caller's, alive until rdx_rows_end returns) filled with pad_id.
 * rows + stage <= max_batch; more than 32 rows + stage need the Vicuna-7B widths; 1 <= cap < max_len. The step's kernel family is that of `rows` rows. */
int rdx_rows_begin(rdx_ctx* ctx, int rows, int stage, int cap /*tokens per request, max*/, int eos_id, int pad_id, int32_t* out_tokens /*device [rows][cap]*/);
/* R prompts (ids / mask / qformer_embs as for rdx_prefill: device, left-padded to T) into the live rows rows_host[0 .. R-1] (HOST; distinct, < rows),
 * enqueued behind the steps so far. 1 <= R <= stage; T + cap <= max_len and <= max_position_embeddings. The target's out_tokens row is cleared to pad_id and
 * holds token 0 in column 0; logits: nullable model-dtype [R][vocab], the prompts' last-position logits. The results of a row are those of
 * rdx_generate on its prompt, bit for bit, whatever its neighbours hold and whenever it arrives. */
int rdx_rows_refill(rdx_ctx* ctx, const int32_t* ids /*dev [R][T], left-padded*/, const int32_t* mask /*nullable*/, int R, int T,
                    const float* qformer_embs /*nullable*/, const int32_t* rows_host /*[R]*/, void* logits /*nullable [R][vocab]*/);
/* n decode steps of all rows, enqueued without a sync: eager launches, or (use_graph) replays of the captured step graph, keyed by (rows, cap, eos, pad,
 * out_tokens, logits). Returns -1 when a live row would pass max_len / max_position_embeddings (host mirror), for n < 1 or n >= max_len, and for logits
 * with n != 1. logits: nullable model-dtype [rows][vocab] of that one step (parked rows: undefined values). */
int rdx_rows_step(rdx_ctx* ctx, int n, int use_graph, void* logits /*nullable [rows][vocab]; only with n == 1*/);
/* Drains the stream, then unfinished_host[rows] (HOST) = the rows' unfinished flags (0: parked, or ended by EOS) and steps_host[rows] (HOST, nullable) =
 * tokens selected so far by each live row (host mirror; 0 for a parked row). A live row seen finished here is parked from the next step on: its tokens stay,
 * and so does its count.
 * Returns -5 when a fused / chained launch reported a hand-off timeout since the last poll (results invalid), like rdx_generate. */
int rdx_rows_poll(rdx_ctx* ctx, int32_t* unfinished_host /*[rows]*/, int32_t* steps_host /*[rows]*/);
/* Parks the live rows rows_host[0 .. n-1] (HOST); their out_tokens rows stay as they are. */
int rdx_rows_park(rdx_ctx* ctx, const int32_t* rows_host, int n);
/* Drains the stream and closes the session. The context is left without a conversation, as after rdx_score: the decode-step and append calls return -1
 * until the next prefill. */
int rdx_rows_end(rdx_ctx* ctx);

/* Data-parallel report generation: every image / report is an independent unit, each rank (one process per GPU)
 * runs encode -> prefill -> decode on its own shard with a full weight replica and NO data-path collective; the generated token ids
 * are gathered once at the end with ONE RCCL all-gather over xGMI. The reference has no inference-time collective (its only
 * distributed code is LAVIS' training DDP, runner_base.py:101-118): this is the addition north_star asks for.
 *   rdx_comm_unique_id  rank 0 creates the 128-byte RCCL id (ncclGetUniqueId); the caller hands it to every rank over any host
 *                       channel (radialog_amd/shard.py uses the launcher's TCP store)
 *   rdx_comm_init       ncclCommInitRank on the context's device; collective: every rank of `world` must call it
 *   rdx_allgather_tokens local int32[rows_local][n] (device) -> global int32[world * rows_local][n] (device), rank-major, enqueued
 *                       on the context's stream (rdx_sync to wait); rows_local and n must be the same on every rank */
typedef struct rdx_unique_id { char internal[128]; } rdx_unique_id;
int rdx_comm_unique_id(rdx_unique_id* id_host);
int rdx_comm_init(rdx_ctx* ctx, const rdx_unique_id* id_host, int rank, int world);
int rdx_allgather_tokens(rdx_ctx* ctx, const int32_t* local, int32_t* global, int rows_local, int n);
int rdx_comm_world(rdx_ctx* ctx);                  /* ranks of the initialised communicator, 0 = none */

/* introspection for tests / benchmarks (the kernel-test, trace and microbenchmark hooks are NOT in this library: include/rdx_hooks.h,
 * librdx_hooks.so, loaded under RDX_DEBUG_HOOKS=1 only) */
int rdx_kv_read(rdx_ctx* ctx, int layer, int which /*0=K,1=V*/, void* dst /*model dtype [B][heads][max_len][D]*/);
int rdx_hidden_read(rdx_ctx* ctx, void* dst /*model dtype [B][hidden]: decoder output rows of the last call*/);
/* fp8 KV cache ("kv_fp8"): rdx_kv_read returns the stored values x' in the model dtype; rdx_kv_read_codes the e4m3 codes [B][heads][max_len][D] bytes and
 * the row exponents [B][heads][max_len] int8 of one layer, both in logical order (device pointers; -1 on a context without the option).
 * rdx_kv_bytes: bytes of the context's KV allocation (caches and, fp8, exponents; < 0 without llama state). */
int rdx_kv_read_codes(rdx_ctx* ctx, int layer, int which /*0=K,1=V*/, void* codes, void* exps);
long long rdx_kv_bytes(rdx_ctx* ctx);
/* average duration (ms) of one hot-path unit, measured with HIP events on the context's stream:
 *   what = 0: one decode step (whole graph) at the current state, `iters` replays
 *   what = 1: the gate/up SwiGLU weight-streaming GEMV of every layer in turn, `iters` sweeps -> ms per launch
 *   what = 2: ... the QKV GEMV, 3: o_proj, 4: down_proj, 5: lm_head, 6: decode attention (re-appends the current KV row);
 *   what = 7: the chained down(l) -> QKV(l+1) launch (decode_chain_k, the batch <= 2 default), measured in situ: `iters` eager
 *             decode steps with an event pair around each of its launches (bracket = launch gap + kernel) -> ms per launch
 *   what + 10: the same unit on layer 0 only (weights stay cache resident)
 *   At batch >= 3 the RMSNorm in front of QKV / gate-up / lm_head is a launch of its own: it runs once, outside the timed region, and
 *   units 1, 2, 5 time the GEMM launches alone. */
int rdx_time(rdx_ctx* ctx, int what, int iters, float* ms_host);
/* The runtime switches of one context. Every switch is one row of one table (radialog_amd/csrc/api_options.hip; for the caller: INTEGRATION.md "Runtime
 * switches": option, environment variable, default, when settable, what it selects). Its environment variable is read once, at rdx_create; after that only
 * rdx_set_option changes it, for this context. A boolean stores value != 0; any other value outside its row's range, an unknown name, and a row that
 * rdx_finalize_weights allocates by ("kv_fp8", "kperm") set after that call return -1 with a message and change nothing. Where a captured step graph holds
 * the old choice it is dropped. No reference counterpart.
 * "kv_fp8" = the decoder's KV cache as an fp8 storage format (0, default: the model dtype; 1: OCP e4m3 codes with one power-of-two exponent
 * byte per cache row of 128 values, radialog_amd/kv8.py). Valid only BEFORE rdx_finalize_weights, which then allocates codes, exponents and one layer of
 * staging rows instead of the 2-byte caches (afterwards: -1 with a message). A stored row IS its dequantised value x' = code 2^e, exactly a value of the
 * model dtype: decode attention over the fp8 cache gives the bits it gives over a model-dtype cache holding x'. The prompt's own attention sees its
 * unquantised K / V (the prompt's logits, token 0 and rdx_score are those of a plain context), a decode step's new token takes part in its own step
 * unquantised and is stored quantised. Rows 1-2 run the generic kernel family (no fused attention + o_proj, no chained launch). Not built on an fp8
 * cache, -1 with a message naming "kv_fp8": rdx_prefill_append / rdx_generate_append (the kept prefix is not held in the model dtype), rdx_beam_search,
 * rdx_rows_begin. Without the option every launch and every output bit is unchanged.
 * At batch 3-16 on the xs16 family rdx_time units 1-5 time THOSE kernels (the RMSNorm is their prologue); max_batch > 32 needs the Vicuna-7B widths
 * (hidden 4096, inter 11008): rdx_finalize_weights refuses other models with more than 32 rows. */
int rdx_set_option(rdx_ctx* ctx, const char* name, int value);
/* what is in force: the value of switch `name` as stored ("kperm" stays -1 where rdx_finalize_weights chose) */
int rdx_get_option(rdx_ctx* ctx, const char* name, int* value);
/* the table's option names in order; NULL past the end */
const char* rdx_option_name(int index);

#ifdef __cplusplus
}
#endif
#endif /* RDX_H */
