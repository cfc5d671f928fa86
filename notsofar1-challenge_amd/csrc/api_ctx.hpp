// Internal header of libcss_mi355.so's host side (the api_*.hip units).  The C ABI is include/css_mi355.h;
// nothing here is exported on purpose.  css_ctx is the handle: the model, its streams and workspaces, and -- through SessState --
// the session the stage entry points see.
// Four owners hold what the library keeps on the GPU: DevBuf (device memory), PinnedBuf (page-locked host memory), Event (a
// hipEvent_t) and std::unique_ptr (a stream's optional parts, api_stream.hpp).  The rule is "members, not lists": a resource is a
// member of the handle, of a stream or of one call's stack and is released with it; no function enumerates what to free.
// HIP streams stay explicit (css_destroy): the handle's own may be the caller's, and the order of synchronise and destroy matters.
#pragma once
#include "../../include/css_mi355.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <dlfcn.h>
#include <mutex>

#include "kernels.hpp"
#include "lsap.hpp"

using namespace css;

// kernel families of the per-launch profile (css_set_profile / css_get_kernel_stats), in the order of the pass
enum ProfCat : int {
    CSS_PROF_DEINTERLEAVE = 0, CSS_PROF_STFT, CSS_PROF_FEATURES, CSS_PROF_LINEAR, CSS_PROF_LAYERNORM, CSS_PROF_ATTENTION,
    CSS_PROF_CONV, CSS_PROF_SCM, CSS_PROF_MVDR_SOLVE, CSS_PROF_BEAMFORM, CSS_PROF_PIT, CSS_PROF_OLA_MASKS, CSS_PROF_GATE,
    CSS_PROF_OLA_STFT, CSS_PROF_ISTFT_GEMM, CSS_PROF_WAVE_OLA, CSS_PROF_ENCODE, CSS_PROF_COUNT
};
static const char* const kProfNames[CSS_PROF_COUNT] = {
    "deinterleave", "stft", "features", "linear_gemm", "layernorm", "attention", "conv_module", "scm", "mvdr_solve",
    "beamform", "pit", "ola_masks", "gate", "ola_stft", "istft_gemm", "wave_ola", "encode_pcm16"};


thread_local extern std::string g_create_error;   // css_last_error(NULL): why the last css_create of this thread failed

// ---- the owners (see the top of this file).  Move-only, a moved-from owner is empty; none has static or thread storage
// duration: the HIP runtime may be gone when such destructors run.
struct DevBuf {   // device memory (allocated by ensure / dev_alloc, api_core.hip)
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { reset(); }
    hipError_t reset() { const hipError_t e = p ? hipFree(p) : hipSuccess; p = nullptr; cap = 0; return e; }
    template <class T = float> T* as() const { return static_cast<T*>(p); }
};

struct PinnedBuf {   // page-locked host memory
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~PinnedBuf() { reset(); }
    hipError_t reset() { const hipError_t e = p ? hipHostFree(p) : hipSuccess; p = nullptr; cap = 0; return e; }
    hipError_t alloc(size_t bytes) {   // (what it held is released first)
        hipError_t e = reset();
        if (e == hipSuccess) e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct Event {   // a hipEvent_t; passes as one wherever an event is recorded, waited for or timed
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { reset(); }
    void reset() { if (e) hipEventDestroy(e); e = nullptr; }
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&e, flags); }
    hipEvent_t get() const { return e; }
    operator hipEvent_t() const { return e; }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_constructible<PinnedBuf>::value && !std::is_copy_constructible<Event>::value &&
              std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_constructible<PinnedBuf>::value &&
              std::is_nothrow_move_constructible<Event>::value, "the owners are move-only");

struct BlockWeights {
    const float *ffi_ln_w, *ffi_ln_b, *ffi_w1, *ffi_b1, *ffi_w2, *ffi_b2;
    const float *att_ln_w, *att_ln_b, *wqkv, *bqkv, *wo, *bo;
    const float *conv_ln_w, *conv_ln_b, *pw, *dw_wt, *dw_b, *bn_alpha, *bn_beta;
    const float *ffo_ln_w, *ffo_ln_b, *ffo_w1, *ffo_b1, *ffo_w2, *ffo_b2;
    const float *fin_ln_w, *fin_ln_b;
};

struct Weights {
    const float *input_bias, *input_scale, *embed_w, *embed_b, *embed_ln_w, *embed_ln_b, *pe_k;
    std::vector<BlockWeights> blocks;
    const float *head_w, *head_b;
};

inline int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
// X holds the planes [C][2F][T_ld] (Re | Im) and, behind them, the phase planes [C][F][T_ld] the analysis transform writes
// with them (kernels.hpp launch_stft_fft): one allocation, so that whatever swaps or re-sizes X takes the phases along
constexpr int X_ROWS_PER_BIN = 3;
struct ncclUniqueId_bytes { char internal[CSS_COMM_ID_BYTES]; };   // ncclUniqueId (rccl.h: 128 opaque bytes, passed by value)
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }


// What belongs to ONE session (recording) on a handle: its plan, its configuration and the device buffers the stages
// after the mask estimator work on.  The handle IS a SessState (the session the stage entry points see); a group of
// queued sessions that shares one estimator batch (run_group) parks the others in css_ctx::slots and swaps them in one
// at a time, so every stage helper keeps addressing `h->X`, `h->plan` ... unchanged.
struct SessState {
    bool has_session = false;
    CssRunCfg cfg{};
    CssPlan plan{};
    int n_ch = 0;
    int64_t n_pad = 0, T_ld = 0;
    bool stft_done = false, perms_done = false, have_override = false;
    bool ph_valid = false;       // the phase planes behind X belong to X (false after css_write_buffer(CSS_BUF_X): the feature kernel forms them itself)
    std::vector<float> w_host;   // segment weights of the session (cfg.w_* point into it)
    DevBuf pcm_cm, X, scm, bfw, sep, costs, perms, mask_st, activity, act_b, act_tmp, act_final, Y, G, wav, wta, pnorm, pit_part;
    DevBuf X_alt;   // run_group: consecutive grouped passes alternate between X and X_alt (the beamformer of pass P reads its
                    // planes on the tail stream while pass P + 1's transform already writes the other set)
    const float* pcm_src = nullptr;       // sample-major PCM on the device for the current session
    bool src16 = false;                   // run_group: pcm_src holds the session's n_ch mono PCM16 planes [C][n] instead (css_run_enqueue_pcm16)
    unsigned int* peak_dev = nullptr;     // max |sample| of the session's PCM as float bits (split_f16.hpp level_gain)
    // the session's masks [(S+1)F][mask_ld], segment s at column s*T: the handle's mask buffer, or -- inside a group -- this
    // session's columns of the group's buffer (the mask head of the shared estimator batch writes all of them at once)
    float* masks_v = nullptr;
    int64_t mask_ld_v = 0;
};

// What css_run_enqueue_handoff / css_run_enqueue_pcm16_handoff ask for beside the waveforms (api_session_handoff.hip): the
// caller's page-locked arrays by their DEVICE addresses -- the kernels of the hand-off store into them.
// The encoder windows a session asks for on top (api_session_window.hip, include/css_mi355_session_window.h): the caller's device
// memory, and its two count arrays by their DEVICE addresses.
struct SessWindowReq {
    bool on = false;
    int32_t width = 0, stride = 0, f16 = 0;
    void* windows = nullptr; int64_t ld = 0, cap_windows = 0;   // [S][cap_windows][n_mels][ld], or null
    void* whole = nullptr; int64_t whole_ld = 0;                // [S][n_mels][whole_ld], or null
    int32_t* n_windows = nullptr; float* window_max = nullptr;  // [S] each
};
// The other tail of a hand-off session (api_nemo_handoff.hip, include/css_mi355_nemo_handoff.h): NeMo's features in place of
// Whisper's.  The ranges and the counts stay SessHandoffReq's; `mel` / `cap_frames` there are unused, and win is off.
struct SessNemoReq {
    bool on = false;
    float preemph = 0.f; int32_t normalize = 1;
    float* mel = nullptr; int64_t cap_frames = 0;       // [S][n_mels][cap_frames]
    float* mean = nullptr; float* stdv = nullptr;       // [S][n_mels] each, or null
};
struct SessHandoffReq {
    bool on = false;
    CssStreamHandoffCfg cfg{};
    SessNemoReq nemo;
    float* mel = nullptr; int64_t cap_frames = 0;       // [S][n_mels][cap_frames]; null (a window session may): no log-mel to the host
    SessWindowReq win;
    int64_t* ranges = nullptr; int32_t cap_ranges = 0;  // [S][cap_ranges][2]
    int64_t* n_frames = nullptr; int32_t* n_ranges = nullptr;
};

// What css_run*_rate ask for beside the session (api_session_rate.hip): the two ratios with their device tables, the counts, and --
// with an output ratio -- where the streams at the output rate go.  Such a session's RunIo / QueuedSession has no sink of its
// own (wav == wav16 == nullptr, cap = the model-rate n_out): its waveforms stay in HBM and leave through session_output_on.
struct SessRate {
    bool on = false, in_on = false, out_on = false;   // a rate session; its input / output side has a ratio other than 1 / 1
    ResampleRatio in{}, out{};
    const float* in_tab = nullptr; const float* out_tab = nullptr;   // the phase tables on the device (css_ctx::rate_tabs)
    int64_t n_in = 0, n_out = 0;   // capture-rate samples per channel; output-rate samples per stream
    float* wav = nullptr; int16_t* wav16 = nullptr; float* peaks = nullptr; int64_t cap = 0;   // (out_on) the caller's [S][cap], peaks [S]
};

// Where the samples of a pass come from and where its result goes (exactly one source; one sink, or -- a queued session that
// only hands off -- none).
struct RunIo {
    const float* pcm_host = nullptr;             // [n][C] float32 in host memory   (css_run)
    const float* pcm_dev = nullptr;              // [n][C] float32 in HBM           (css_run_device)
    const int16_t* const* planes_host = nullptr; // C mono PCM16 planes in host memory (css_run_pcm16)
    float* wav_host = nullptr;                   // [S][cap] float32
    float* wav_dev = nullptr;
    int16_t* wav16_host = nullptr;               // [S][cap] peak-normalised PCM16
    float* peaks_host = nullptr;
    int64_t cap = 0;
    bool enqueue_only = false;                   // css_run_enqueue: return once everything is on the streams
    const SessHandoffReq* ho = nullptr;          // a queued session that also hands off: behind the waveforms, on their stream
    const SessRate* rate = nullptr;              // a rate session: with in_on, pcm_host / planes_host are at the capture rate (rate->n_in samples)
    bool level_done = false;                     // pcm_dev: the recording's level is already in the level word (the ingest kernel wrote it)
    // host to host: float PCM -> float waveforms (pcm, wav) or PCM16 planes -> PCM16 streams and their peaks (planes, wav16, peaks)
    static RunIo host(const float* pcm, const int16_t* const* planes, float* wav, int16_t* wav16, float* peaks, int64_t cap,
                      bool enqueue_only = false) {
        RunIo io;
        io.pcm_host = pcm; io.planes_host = planes; io.wav_host = wav; io.wav16_host = wav16; io.peaks_host = peaks;
        io.cap = cap; io.enqueue_only = enqueue_only;
        return io;
    }
    static RunIo device(const float* pcm, float* wav, int64_t cap) {
        RunIo io;
        io.pcm_dev = pcm; io.wav_dev = wav; io.cap = cap;
        return io;
    }
};

struct StreamState;   // api_stream.hpp: a streamed session and what its hand-off shares on a handle; owned through
struct HandoffCtx;    // css_stream_close / stream_destroy_all (api_stream.hip), where the order of synchronise and delete matters

struct css_ctx : SessState {
    CssModelDesc d{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int max_batch = 64;
    int Kp = 0, KIp = 0;
    DevBuf blob;                 // the weights as uploaded (w points into it)
    Weights w;
    // Linear-layer arithmetic.  Default (round 6): float32 operands on the float32 matrix instruction (gemm_f32.hip) -- the
    // reference's own operand precision (conformer.py:137-150 runs torch.nn.Linear in float32).  Opt-in, after
    // css_set_linear_mode(h, CSS_LINEAR_SPLIT_F16): split-f16 operands on the f16 matrix cores (22-bit operands, gemm_split*.hip).
    bool split = false;
    bool split_ok = true;        // false: a weight lies outside the split-f16 operand range, CSS_LINEAR_SPLIT_F16 is refused
    DevBuf wsplit;               // split-f16 images of the Linear weights, at the blob's own offsets
    DevBuf dft_split;            // split-f16 image of dft_inv_t (row-major)
    DevBuf wfrag;                // exact float32 mode: the Linear weights in gemm_f32.hip's fragment order (same offsets as blob)
    DevBuf dft_tiled;            // ... and in the tile-major layout of the weights-direct GEMM (whole-meeting synthesis)
    DevBuf head_tiled;           // the mask head's weights in that layout (rows rounded up to 32; wsplit keeps the row-major image)
    DevBuf pe_frag[2];           // relative-position rows in attention-operand order for segment length pe_frag_T
    int pe_frag_T[2] = {0, 0};   // ([0] from the float32 table, [1] from the split-f16 one; encoder.hip pe_fragments_kernel)
    DevBuf stft_tab;             // window and twiddles of the analysis FFT (stft.hip)
    bool fft512 = true;          // frame_len 512 / hop 256 / 257 bins: the FFT kernel and the pipelined schedules; else the generic forms
    DevBuf dft_fwd;              // generic analysis: [2F][Lp] = (cos | -sin)(2 pi f n / N) * window[n], n < frame_len (zero beyond)
    int Lp = 0, ovl = 2;         // frame_len rounded up to 32; frames over an output sample = ceil(frame_len / hop)
    DevBuf dft_inv_t;            // [frame_len][KIp]

    // shared by the sessions of a handle: upload staging, the estimator's activations, the mask buffer, small tables
    std::vector<float> w_on_device;   // what segw holds (uploaded when a session's windows differ)
    DevBuf pcm_in, feat, hx, hu, ht, qkv, qkf, ctxb, masks, segw, stage, in16, pcm_f, enc, level, mel_tab, mel_work;
    // the hand-off of queued sessions (api_session_handoff.hip): the DFT matrix with BOTH filterbanks (a queue may alternate
    // between them, so neither is ever rebuilt), and one set of work buffers -- tails are serial on their stream
    DevBuf sh_tab, sh_work;
    DevBuf nemo_tab;    // a NeMo session's tables (api_nemo_handoff.hip): the [514][512] analysis matrix and both banks at 257 bins
    PinnedBuf sh_pin;   // css_handoff_logmel_all into pageable arrays: the kernels' destination, copied out after the synchronise
    // sessions of a queued group other than the active one (run_group)
    static constexpr int MAX_GROUP = 8;
    std::vector<SessState> slots;
    int group_limit = MAX_GROUP;      // css_set_queue_group: sessions merged into one estimator batch (1: none)
    // Second lane of the mask estimator: segments are independent through the whole network, so a batch is cut in `lanes`
    // parts that run as independent chains of kernels on as many streams.  One chain alone leaves the GPU idle in every
    // launch's prologue and epilogue (its waves are parked 51 % of the time, profiles/); two or three chains drift out of
    // phase and fill each other's bubbles (measured: 6.9 -> 6.4 ms per 60 s meeting with two).  Results do not change: every
    // kernel is batch invariant.  css_set_lanes(h, 1) turns it off.
    // (css_set_lanes: 1..4, default 3; lane 0 is `stream` with the buffers above)
    static constexpr int MAX_LANES = 4;
    int lanes = 3;
    hipStream_t lane_stream[MAX_LANES] = {};   // [0] unused
    Event ev_fork, ev_join[MAX_LANES];
    DevBuf lfeat[MAX_LANES], lhx[MAX_LANES], lhu[MAX_LANES], lht[MAX_LANES], lqkv[MAX_LANES], lqkf[MAX_LANES], lctx[MAX_LANES];   // [0] unused
    int64_t last_batch_tokens = 0;
    int mel_bands = 0;                    // the filterbank mel_tab holds (0: none yet)
    // range check of the split-f16 operand format (split_f16.hpp): a device word set when the stitched activity or the
    // waveforms hold a non-finite value, mirrored into page-locked host memory at the end of every pass
    DevBuf range_flag_dev;           // (64 bytes; word 0 is the flag)
    PinnedBuf range_flag_host;
    bool range_fallback = true;      // repeat such a pass on the exact float32 kernels (else: CSS_ERR_RANGE)
    int64_t range_fallbacks = 0;     // passes repeated so far
    int range_last = 0;              // the last pass hit the range limit
    // PCIe pieces of css_run* travel on their own stream, beside the kernels: the upload of the samples a lane's segments
    // read is followed by that lane's analysis transform and mask-estimator chain while the next piece is in flight, and
    // finished ranges of the output leave while the last ranges are still being synthesised.
    hipStream_t copy_stream = nullptr;
    // css_run*: what follows the mask estimator (covariances and beamformer per segment on the lanes, then -- in segment
    // order, on this stream -- stitching costs, the permutation scan, overlap-add, gate, synthesis) trails the lanes unit
    // by unit instead of waiting for the last segment of the recording
    hipStream_t tail_stream = nullptr;
    // schedule choices of that pipeline (css_set_tuning; defaults = what measured best, A/B on one box: tools/ab_tuning.py)
    int tune[CSS_TUNE_COUNT] = {1, 0, 0, 1, 0, 2, 1, 0, 1, 0, 24576, 14000};
    const void* mapped_key = nullptr;   // last page-locked output buffer looked up, and its device address
    void* mapped_val = nullptr;
    // css_run_enqueue / css_wait: passes enqueued and not yet waited for
    int queued = 0;
    // queued passes overlap: pass P's samples cross PCIe while pass P - 1's kernels run, and P - 1's stitching / synthesis /
    // download run beside P's estimator.  The sample buffer and the level word alternate (pass parity); `pcm_free[b]` =
    // the last transform of the pass that used sample buffer b; `tail_end` = the end of the last queued pass's tail
    // (untimed events, created with the handle)
    int64_t pass_no = 0;
    Event pcm_free[2];
    Event pass_end[4];     // ends of the last four queued passes (back-pressure)
    Event level_free[2];   // end of the tail of the pass that used level word b (its last reader)
    Event tail_end;
    bool tail_pending = false;
    bool piped_now = false;   // run_once -> begin_impl: the level word is cleared on the copy stream, not here
    int last_piped = -1;      // overlap mode of the last queued pass (-1: nothing queued): a queue never mixes modes un-drained
    // One session of css_run_enqueue / css_run_enqueue_pcm16: the call's arguments, with its own copy of the three stitching
    // windows and of the plane pointers (the caller may free its own; it keeps the samples valid and the output untouched
    // until css_wait anyway).  PCM16 session: planes set, pcm == wav == nullptr.
    struct QueuedSession {
        const float* pcm; int64_t n; int32_t n_ch; CssRunCfg cfg; float* wav; int64_t cap;
        std::vector<const int16_t*> planes; int16_t* wav16; float* peaks;
        float* wav_mapped;      // device address of the page-locked output (nullptr: pageable, or never looked up)
        SessHandoffReq ho;      // css_run_enqueue*_handoff (wav may then be nullptr: log-mel only)
        SessRate rate;          // css_run*_rate: n is the MODEL-rate count, pcm / planes hold rate.n_in capture-rate samples
        std::vector<float> w;   // w_first | w_mid | w_last of cfg
        QueuedSession(const float* pcm_, const int16_t* const* planes_, int64_t n_, int32_t n_ch_, const CssRunCfg& c, float* wav_,
                      int16_t* wav16_, float* peaks_, int64_t cap_, float* mapped_)
            : pcm(pcm_), n(n_), n_ch(n_ch_), cfg(c), wav(wav_), cap(cap_), wav16(wav16_), peaks(peaks_), wav_mapped(mapped_) {
            if (planes_) planes.assign(planes_, planes_ + n_ch_);
            const size_t T = (size_t)std::max(c.segment_frames, 0);
            w.resize(3 * T);
            if (T && c.w_first && c.w_mid && c.w_last) {
                std::memcpy(w.data(), c.w_first, T * sizeof(float));
                std::memcpy(w.data() + T, c.w_mid, T * sizeof(float));
                std::memcpy(w.data() + 2 * T, c.w_last, T * sizeof(float));
            }
        }
        bool pcm16() const { return !planes.empty(); }
        CssRunCfg own_cfg() const {   // cfg with its window pointers at this record's copies
            CssRunCfg c = cfg;
            const size_t T = w.size() / 3;
            c.w_first = w.data(); c.w_mid = w.data() + T; c.w_last = w.data() + 2 * T;
            return c;
        }
        RunIo io(bool enqueue_only) const {
            RunIo io = RunIo::host(pcm, pcm16() ? planes.data() : nullptr, wav, wav16, peaks, cap, enqueue_only);
            io.ho = ho.on ? &ho : nullptr;
            io.rate = rate.on ? &rate : nullptr;
            return io;
        }
        // may the two share an estimator batch: one segmentation, the same three windows bit for bit
        bool groups_with(const QueuedSession& o) const {
            return cfg.segment_frames == o.cfg.segment_frames && cfg.hop_frames == o.cfg.hop_frames && w.size() == o.w.size() &&
                   std::memcmp(w.data(), o.w.data(), w.size() * sizeof(float)) == 0;
        }
    };
    // sessions put on the streams since the last css_wait: a queued pass that left the split-f16 range is repeated from
    // them on the exact float32 kernels
    std::vector<QueuedSession> queue_log;
    // css_run_enqueue: sessions accepted and not yet on the streams -- they wait for company: sessions of one segment
    // length are merged into ONE estimator batch (run_group) as long as their segments fit max_batch_segments; flush_pending
    // moves them into queue_log
    std::vector<QueuedSession> pending;
    int64_t pending_segments = 0;
    // css_wait_sessions: one event per session put on the streams since the last css_wait, in queue order, recorded behind the
    // session's last output copy (nullptr: the session had finished inside its call)
    std::vector<hipEvent_t> sess_done;
    std::vector<Event> sess_ev_pool;
    size_t sess_ev_used = 0;
    void* comm = nullptr;          // ncclComm_t of css_comm_init (RCCL, loaded lazily)
    int comm_ranks = 0, comm_rank = -1;
    // css_upload_range: further pieces of the recording on their way over PCIe (copy stream); css_stage_stft_range makes
    // the handle's stream wait for exactly the pieces its frames read
    struct PendingUpload { int64_t s_lo, s_hi; hipEvent_t landed; };
    std::vector<PendingUpload> uploads;
    std::vector<Event> ev_pool;   // untimed events of the pipeline (uploads landed, planes ready, ranges finished)
    size_t ev_pool_used = 0;

    // timing
    Event ev[10];
    CssTimings tim{};
    // css_set_profile: every kernel launch of a pass is bracketed by a pair of HIP events on its stream (one lane, so
    // that the pairs are ordered); durations are summed per kernel family (css_get_kernel_stats)
    bool profile_gemm = false;
    struct ProfEvent { Event a, b; int cat = 0; };
    std::vector<ProfEvent> prof_events;
    size_t prof_used = 0;
    size_t prof_reduced = 0;   // brackets already summed into prof_ms (a staged session has no closing call that does it)
    double gemm_flops = 0.0;
    float prof_ms[CSS_PROF_COUNT] = {};
    int32_t prof_launches[CSS_PROF_COUNT] = {};
    // what an event pair measures with NOTHING between the two records (css_set_profile calibrates it): the part of every
    // bracketed launch that is the bracket, not the kernel
    float prof_pair_ms = 0.f;
    int32_t prof_pairs = 0;
    FeatOpts feat_opts{};   // css_set_feature_options (css_create: the shipped configuration)
    StreamState* streams[CSS_MAX_STREAMS] = {};   // css_stream_open: open streams (api_stream.hpp), by id
    HandoffCtx* handoff = nullptr;   // api_stream_handoff.hip: what the hand-off of streams shares on this handle, made on first use
    int32_t stream_out_launches = 0, stream_out_rounds = 0;   // api_stream.hip stream_round: the output kernel in the last push / finish call
    // css_run*_rate (api_session_rate.hip): the phase tables of the ratios met so far (never rebuilt, never moved: queued sessions
    // hold their addresses), the output edge's buffers (level words | float rows | PCM16 rows; tails are serial on their stream),
    // and the running counts of css_session_rate_stats
    struct RateTab { int up, down; DevBuf tab; };
    std::vector<std::unique_ptr<RateTab>> rate_tabs;
    DevBuf rate_out;
    int64_t rate_ingest_launches = 0, rate_output_launches = 0, rate_sessions = 0;
    int64_t window_launches = 0, window_sessions = 0;   // css_session_window_stats: launches of the window kernel, sessions that asked for windows
    DevBuf stream_masks;   // api_stream.hip: the mask head's output for one estimator batch of streamed segments (never `masks`:
                           // the handle's own session keeps its bits between two pushes)

    std::string err;
};

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(h, CSS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)


// ---- api_core.hip
int fail(css_ctx* h, int code, const std::string& msg);
hipError_t dev_alloc(DevBuf& b, size_t bytes);
int ensure(css_ctx* h, DevBuf& b, size_t bytes, bool zero = false);
int64_t bind_weights(const CssModelDesc& d, const float* base, Weights* w);
const char* validate_desc(const CssModelDesc& d);
void exact_cs(int64_t k, int N, double* c, double* s);
bool deal_streams(hipStream_t main, hipStream_t lane[4], hipStream_t* copy, hipStream_t* tail);
int plan_impl(const CssModelDesc& d, const CssRunCfg& cfg, int64_t n, CssPlan* p);
void gemm(css_ctx* h, const GemmArgs& g, hipStream_t st);
GemmArgs linear(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc, int M, int N, int K, int act);
StitchArgs stitch_args(css_ctx* h);
MvdrArgs mvdr_args(css_ctx* h, int64_t lo, int nseg);
int64_t batch_cap(const css_ctx* h, int T);
int ensure_activations(css_ctx* h, int64_t nb, int T);
int make_split_weights(css_ctx* h);
int make_frag_weights(css_ctx* h);
int check_session(css_ctx* h);
int upload_analysis_matrix(css_ctx* h, int window);
bool analysis_transform(css_ctx* h, const float* x, int64_t x_stride, int C, int64_t t_lo, int64_t t_hi, float* out, int64_t row_ld,
                        hipStream_t st, float* phase, bool* phase_done);

// ---- api_stages.hip
// Where one batched pass of the mask estimator reads its spectra and writes its masks.
struct GroupSess { const float* X; int64_t T_ld, stft_frames; int64_t off; int n; const float* PH; };   // a session's planes (+ phase planes); its segments are the batch's [off, off + n)
struct MaskIo {
    const float* X; int64_t T_ld; int64_t stft_frames; int hop; int T;   // planes [C][2F][T_ld], segment s at s*hop
    float* masks; int64_t mask_ld;                                       // [(S+1)F][mask_ld], segment s at column s*T
    // a batch over the segments of SEVERAL sessions (run_group): the features of batch segment c come from the session
    // that holds it, everything behind them is one [segments * T, .] problem; X / T_ld / stft_frames above are unused
    const std::vector<GroupSess>* group = nullptr;
    const float* PH = nullptr;   // phase planes [C][F][T_ld] beside X (nullptr: the feature kernel forms the phases itself)
};
struct LaneSplit { int nl, per; };   // how a batch of segments is cut into lanes: `nl` chains of `per` segments (the last one shorter)
using LanePrep = std::function<int(int64_t, int, hipStream_t)>;
using LanePost = LanePrep;   // post(first segment, count, stream): enqueued at the END of each lane's chain
int check_run_args(css_handle_t h, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg, CssPlan* plan_out);
int begin_impl(css_handle_t h, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg);
int upload_pcm(css_handle_t h, const float* pcm_host, int64_t s_lo, int64_t s_hi, hipStream_t st);
int64_t covered_end(const css_ctx* h);
int64_t peak_len(const css_ctx* h, int64_t s_lo, int64_t s_hi);
int stft_frames(css_ctx* h, int64_t t_lo, int64_t t_hi, const int16_t* planes16, hipStream_t st);
int masknet_lane(css_ctx* h, const MaskIo& io, int64_t s0, int nb, int lane, int ph_lo, int ph_hi, bool concurrent = false);
LaneSplit lane_split(const css_ctx* h, int nb, int T);
int64_t batch_len(int64_t n, int64_t cap);
int masknet_batch(css_ctx* h, const MaskIo& io, int64_t s0, int nb, const LanePrep& prep, const LanePost& post, hipEvent_t before_head = nullptr);
int masknet_batch(css_ctx* h, const MaskIo& io, int64_t s0, int nb);
int mvdr_on(css_ctx* h, int64_t seg_lo, int64_t seg_hi, hipStream_t st);
void pit_costs_on(css_ctx* h, int64_t b_lo, int64_t b_hi, hipStream_t st);
void pit_scan_on(css_ctx* h, int64_t b_lo, int64_t b_hi, hipStream_t st);
int check_frames(css_ctx* h, int64_t t_lo, int64_t t_hi);
void istft_gemm_on(css_ctx* h, int64_t f_lo, int64_t f_hi, hipStream_t st);
void wave_ola_on(css_ctx* h, int64_t f_lo, int64_t f_hi, int64_t q_lo, int64_t q_hi, float* out, int64_t out_ld, int64_t out_q0, hipStream_t st);
int istft_impl(css_ctx* h, int64_t f_lo, int64_t f_hi, int64_t q_lo, int64_t q_hi, float* out, int64_t out_ld, int64_t out_q0, hipStream_t st);

// Sample ranges of [a, b) that the gate keeps, appended to `reg` (pairs; a range that touches reg's last one extends it):
// act[i] is the gate byte of frame t0 + i, frames below t_known are known; a run of active frames [t, e) keeps the samples
// [max(t - pad, 0) hop, min((e - 1 + pad) hop + N, n_out)).  The frames that can keep a sample of [a, b) must be known.
// css_handoff_logmel asks for [0, n_out) of a finished pass, a stream for the samples a push decided.
inline void handoff_kept_ranges(const uint8_t* act, int64_t t0, int64_t t_known, int pad, int hop, int N, int64_t a, int64_t b,
                                int64_t n_out, std::vector<int64_t>& reg) {
    const int64_t t_lo = std::max<int64_t>(std::max<int64_t>(a / hop - pad - N / hop, 0), t0);
    const int64_t t_hi = std::min<int64_t>(t_known, (b + hop - 1) / hop + pad);
    for (int64_t t = t_lo; t < t_hi;) {
        if (!act[(size_t)(t - t0)]) { ++t; continue; }
        int64_t e = t;
        while (e < t_hi && act[(size_t)(e - t0)]) ++e;
        const int64_t ra = std::max(std::max<int64_t>(t - pad, 0) * hop, a);
        const int64_t rb = std::min(std::min<int64_t>((e - 1 + pad) * hop + N, n_out), b);
        if (rb > ra) {
            if (!reg.empty() && ra <= reg.back()) reg.back() = std::max(reg.back(), rb);
            else { reg.push_back(ra); reg.push_back(rb); }
        }
        t = e;
    }
}

// ---- api_stream.hip
void stream_destroy_all(css_ctx* h);
int stream_open_count(const css_ctx* h);

// ---- api_queue.hip
hipEvent_t pool_event(css_ctx* h);
void* mapped_host(const void* p);
int enqueue_impl(css_handle_t h, const float* pcm_host, const int16_t* const* planes, int64_t n_samples, int32_t n_ch,
                 const CssRunCfg* cfg, float* wav_host, int16_t* wav16, float* peaks, int64_t cap, const SessHandoffReq* ho = nullptr,
                 const SessRate* rate = nullptr);
int run_impl(css_handle_t h, int64_t n, int32_t n_ch, const CssRunCfg* cfg, const RunIo& io);
int waveforms_out(css_ctx* h, const float* src, int64_t src_ld, float* wav, int64_t cap, int64_t a, int64_t b, hipStream_t st);

// ---- api_session_rate.hip
// a rate session's view of its own sink: the caller's arrays move into q.rate when the output side has a ratio
void session_rate_adopt(css_ctx::QueuedSession& q, const SessRate& rate, int64_t n_out_model);
// the output edge's buffers for a session of this rate (before the first launch of the pass or group: ensure may wait)
int session_rate_prepare(css_ctx* h, const SessRate& r);
// bytes of the capture-rate recording, and the whole ingest of ONE session on `st`: upload to `staging`, the kernel -> dst
size_t session_rate_capture_bytes(const SessRate& r, int n_ch, bool pcm16);
int session_rate_upload(css_ctx* h, const SessRate& r, const float* pcm, const int16_t* const* planes, int n_ch, void* staging, hipStream_t st);
SessionIngestJob session_rate_job(const SessRate& r, bool pcm16, int n_ch, const void* staging, float* dst, int64_t n_model, int64_t n_peak,
                                  unsigned int* level);
int session_rate_ingest(css_ctx* h, const SessionIngestJob* jobs, int n, hipStream_t st);
// the output edge of the handle's current session on `st`: wav [S][wav_ld] in HBM -> the caller's arrays at the output rate
int session_output_on(css_ctx* h, const float* wav, int64_t wav_ld, const SessRate& r, hipStream_t st);

// ---- api_session_handoff.hip
// the handle's tables and work buffers for a session of this plan (before the first launch of the pass or group: ensure may wait)
int session_handoff_prepare(css_ctx* h, const CssPlan& pl, const SessHandoffReq& r);
// the five steps for the handle's current session on `st`, reading its gate bytes and the waveforms wav [S][wav_ld] in HBM
int session_handoff_on(css_ctx* h, const float* wav, int64_t wav_ld, const SessHandoffReq& r, hipStream_t st);
// The checks and the body of the two kinds of entry points, shared with api_session_window.hip (mel_optional: out->mel_host may
// be NULL).  *_check refuse what the header says, with nothing allocated, queued or written; on CSS_OK *frames is the session's
// frame bound.  session_handoff_all_run: `win` holds HOST addresses of its count arrays (pageable ones are staged like `out`'s).
struct CssSessionHandoffOut;   // include/css_mi355_session_handoff.h
int session_handoff_enqueue_check(css_ctx* h, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg,
                                  const CssSessionHandoffOut* out, bool mel_optional, SessHandoffReq* req, int64_t* n_out, int64_t* frames);
int session_handoff_all_check(css_ctx* h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg,
                              const CssSessionHandoffOut* out, bool mel_optional, int64_t* frames);
int session_handoff_all_run(css_ctx* h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out,
                            const SessWindowReq* win);
// ---- api_nemo_handoff.hip: session_handoff_prepare / session_handoff_on hand a request with nemo.on over to these
int nemo_handoff_prepare(css_ctx* h, const CssPlan& pl, const SessHandoffReq& r);
int nemo_handoff_on(css_ctx* h, const float* wav, int64_t wav_ld, const SessHandoffReq& r, hipStream_t st);
// css_ctx::nemo_tab, built on first use, and the bank of n_mels (80 / 128) in it; the matrix is at its start
int nemo_ensure_tables(css_ctx* h);
const float* nemo_bank(const css_ctx* h, int n_mels);
void reduce_profile(css_ctx* h);


// Scope around one kernel launch: with the profile on, an event pair on the launch's stream, tagged with its family.
struct Prof {
    css_ctx* h; hipStream_t st; hipEvent_t stop = nullptr;
    Prof(css_ctx* h_, int cat, hipStream_t st_) : h(h_), st(st_) {
        if (!h->profile_gemm) return;
        if (h->prof_used == h->prof_events.size()) {
            css_ctx::ProfEvent e;
            e.a.create();
            e.b.create();
            h->prof_events.push_back(std::move(e));
        }
        css_ctx::ProfEvent& e = h->prof_events[h->prof_used++];
        e.cat = cat;
        hipEventRecord(e.a, st);
        stop = e.b;
    }
    ~Prof() { if (stop) hipEventRecord(stop, st); }
};
#define CSS_PROF(cat, st) Prof prof_scope_(h, cat, st)

// queued passes (css_run_enqueue) finish before anything else touches the handle's state or buffers
#define CSS_DRAIN(h)                                                  \
    do {                                                              \
        if ((h) && ((h)->queued || !(h)->pending.empty())) {          \
            const int rc_drain_ = css_wait(h);                        \
            if (rc_drain_ != CSS_OK) return rc_drain_;                \
        }                                                             \
    } while (0)

