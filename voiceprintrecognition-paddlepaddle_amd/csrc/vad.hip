// Energy voice-activity detection for speaker diarization: the speech regions of a ragged batch of recordings, found on the device.
// No reference call site: an extension standing in for yeaudio's model-based AudioSegment.vad (speaker_diarization.py:37), which has no
// weights here (docs/vad.md has the method and the contract).  f32 throughout.
//
// vp_vad_frame_db_f32   frame_db_kernel: grid (tiles, recordings).  A workgroup stages the samples of up to 64 snip-edge frames in LDS
//                       (each sample is read from HBM once although it belongs to win / hop frames), then a wave per frame: the frame's
//                       mean, then the mean square of the mean-free, pre-emphasised samples -- two passes over LDS, so a large DC offset
//                       under a quiet signal costs nothing -- and e = 10 log10(max(p, 1e-10)), the logarithm in float64.
// vp_vad_regions_f32    regions_kernel: one workgroup per recording.
//                         1. fl and pk, two order statistics of e, by ONE radix selection on vp_order_key(e): four 8-bit digits, both
//                            ranks counted in the same walk into integer LDS histograms (COPIES per rank); exact, no sort, no
//                            interpolation.
//                         2. on / off in f32, each operation rounded on its own.
//                         3. all waves: 64 frames per wave step, two ballots -> the word of speech-decisive frames (e >= on) and the word
//                            of silence-decisive ones (e < off, and every position past the end) into the workspace.
//                         4. wave 0: 64 words (4096 frames) per step.  A lane resolves the hysteresis inside its word with scan64 -- the
//                            scan of x[t] = g[t] | (p[t] & x[t-1]), g = speech-decisive, p = undecided -- the 64 words' (last state,
//                            all undecided) pairs go through the same scan64 by ballot, and the carry of the step before closes it.
//                            The state words are never stored: their edges (state != state of the frame before) are the run starts and
//                            ends, which the wave walks in order through a small state machine -- gap fill, short-run removal, padding,
//                            merging -- that writes the regions.
// Integer counts only, no float atomics, no spinning, nothing depends on arrival order: two runs give the same bits.
// Both entry points read the B + 1 offsets back once (a few bytes, one stream synchronisation) to check them and size the grid.
#include <vector>

#include "common.h"

namespace {

constexpr int MAX_WIN = 4096;
constexpr int TILE_FLOATS = 12288;      // 48 KB of samples per workgroup
constexpr int TILE_FRAMES = 64;
constexpr int MAX_B = 65535;            // grid.y
constexpr int COPIES = 8;               // of the selection histograms

__host__ __device__ inline int num_frames(long long n, int win, int hop) { return n < win ? 0 : (int)(1 + (n - win) / hop); }

// the B + 1 device offsets on the host; non-decreasing from a non-negative start, else false
int read_offsets(vp_ctx* ctx, const int32_t* dev, int B, std::vector<int32_t>& host, hipStream_t st) {
    host.resize((size_t)B + 1);
    VP_HIP(ctx, hipMemcpyAsync(host.data(), dev, ((size_t)B + 1) * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(ctx, hipStreamSynchronize(st));
    if (host[0] < 0) return VP_EINVAL;
    for (int b = 0; b < B; ++b)
        if (host[b + 1] < host[b]) return VP_EINVAL;
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------ stage A: waveform -> frame energies
struct FrameArgs {
    const float* wave;
    const int32_t* offsets;             // [B + 1] samples
    const int32_t* frame_offsets;       // [B + 1] frames
    int win, hop, tile_frames;
    float preemph;
    float* e;
};

// grid (tiles of tile_frames frames, recordings), 256 threads; tiles beyond a recording's last frame have nothing to do
__global__ __launch_bounds__(256) void frame_db_kernel(const FrameArgs a) {
    __shared__ float s[TILE_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.y;
    const long long first = a.offsets[b];
    const int F = num_frames((long long)a.offsets[b + 1] - first, a.win, a.hop);      // the host checked frame_offsets against it
    const float* x = a.wave + first;
    float* e = a.e + a.frame_offsets[b];
    const float inv = 1.f / (float)a.win;
    for (int t0 = blockIdx.x * a.tile_frames; t0 < F; t0 += gridDim.x * a.tile_frames) {
        const int nf = F - t0 < a.tile_frames ? F - t0 : a.tile_frames;
        const int span = (nf - 1) * a.hop + a.win;          // <= TILE_FLOATS by the choice of tile_frames; ends inside the recording
        const float* src = x + (long long)t0 * a.hop;
        __syncthreads();                                    // the frames of the tile before are done with s
        for (int i = tid; i < span; i += 256) s[i] = src[i];
        __syncthreads();
        for (int f = w; f < nf; f += 4) {                   // wave-uniform
            const float* fr = s + f * a.hop;
            float sum = 0.f;
            for (int i = lane; i < a.win; i += 64) sum += fr[i];
            const float mean = vp_wave_sum(sum) * inv;
            float sq = 0.f;
            for (int i = lane; i < a.win; i += 64) {
                const float y = (fr[i] - mean) - a.preemph * (fr[i ? i - 1 : 0] - mean);
                sq += y * y;
            }
            const float p = fmaxf(vp_wave_sum(sq) * inv, 1e-10f);
            if (lane == 0) e[t0 + f] = (float)(10.0 * log10((double)p));
        }
    }
}

// ------------------------------------------------------------------------------------------------ stage B: frame energies -> regions
struct RegionArgs {
    const float* e;
    const int32_t* frame_offsets;       // [B + 1]
    float floor_pct, peak_pct, margin_db, onset, offset;
    int min_gap, min_speech, pad, cap;
    float* thr;                         // [B][4]: fl, pk, on, off
    int32_t* counts;                    // [B]
    int32_t* regions;                   // [B][cap][2]
    unsigned long long* words;          // workspace: per recording F / 64 + 1 speech-decisive words, then as many silence-decisive ones
    long long total_words;              // of one kind, all recordings
};

__device__ __forceinline__ float key_value(unsigned key) {       // vp_order_key's inverse
    return __uint_as_float(key >> 31 ? key ^ 0x80000000u : ~key);
}

// inclusive scan of x[t] = g[t] | (p[t] & x[t-1]) over the 64 bits, x[-1] = 0: g becomes x, p becomes "p holds at every bit up to t"
// (where the value before bit 0 would come through)
__device__ __forceinline__ void scan64(unsigned long long& g, unsigned long long& p) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        g |= p & (g << d);
        p &= (p << d) | ((1ull << d) - 1ull);
    }
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return (unsigned long long)hi << 32 | lo;
}

// rules 5 - 8 over the speech runs in ascending order, every lane of the wave alike (lane 0 writes)
struct RunWalk {
    long long cur_a = -1, cur_b = 0;    // the run being grown by gap fill
    long long out_a = -1, out_b = 0;    // the padded region being grown by merging
    int count = 0;

    __device__ __forceinline__ void emit(const RegionArgs& a, int32_t* regions, bool writer) {
        if (out_a < 0) return;
        if (writer && count < a.cap) {
            regions[2 * count + 0] = (int32_t)out_a;
            regions[2 * count + 1] = (int32_t)out_b;
        }
        ++count;
    }
    __device__ __forceinline__ void close(const RegionArgs& a, long long F, int32_t* regions, bool writer) {
        if (cur_a < 0 || cur_b - cur_a < a.min_speech) return;
        const long long pa = cur_a - a.pad > 0 ? cur_a - a.pad : 0, pb = cur_b + a.pad < F ? cur_b + a.pad : F;
        if (out_a >= 0 && pa <= out_b) {
            out_b = pb;
        } else {
            emit(a, regions, writer);
            out_a = pa;
            out_b = pb;
        }
    }
    __device__ __forceinline__ void run(const RegionArgs& a, long long F, int32_t* regions, bool writer, long long ra, long long rb) {
        if (cur_a >= 0 && ra - cur_b < a.min_gap) {
            cur_b = rb;
        } else {
            close(a, F, regions, writer);
            cur_a = ra;
            cur_b = rb;
        }
    }
};

// grid (recordings), 1024 threads
__global__ __launch_bounds__(1024) void regions_kernel(const RegionArgs a) {
    __shared__ unsigned hist[2][COPIES][256];      // a copy per lane % COPIES: frames of one level share a digit, and a wave's atomics
                                                    // on one word are served one after the other
    __shared__ unsigned prefix[2], left[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    const int f0 = a.frame_offsets[b], F = a.frame_offsets[b + 1] - f0;
    float* thr = a.thr + 4 * (size_t)b;
    if (F <= 0) {                       // uniform
        if (tid < 4) thr[tid] = 0.f;
        if (tid == 0) a.counts[b] = 0;
        return;
    }
    const float* e = a.e + f0;

    // 1. the two order statistics: rank counted from the smallest, digit by digit from the top
    if (tid < 2) {
        prefix[tid] = 0u;
        const double pct = (double)(tid ? a.peak_pct : a.floor_pct);
        long long k = (long long)floor(pct * (double)(F - 1));
        left[tid] = (unsigned)(k < 0 ? 0 : k > F - 1 ? F - 1 : k);
    }
    for (int top = 32; top > 0; top -= 8) {
        const int sh = top - 8;
        for (int i = tid; i < 2 * COPIES * 256; i += 1024) (&hist[0][0][0])[i] = 0u;
        __syncthreads();                // and the prefixes
        const unsigned p0 = prefix[0], p1 = prefix[1];
        for (int t = tid; t < F; t += 1024) {
            const unsigned key = vp_order_key(e[t]), d = (key >> sh) & 255u;
            const bool all = top == 32;
            if (all || (key >> top) == (p0 >> top)) atomicAdd(&hist[0][lane % COPIES][d], 1u);
            if (all || (key >> top) == (p1 >> top)) atomicAdd(&hist[1][lane % COPIES][d], 1u);
        }
        __syncthreads();
        if (tid < 512) {                // the copies of a digit into copy 0
            unsigned n = 0u;
            for (int c = 0; c < COPIES; ++c) n += hist[tid >> 8][c][tid & 255];
            hist[tid >> 8][0][tid & 255] = n;
        }
        __syncthreads();
        if (tid < 2) {                  // the first digit, from the smallest up, at which the count passes the rank
            const unsigned k = left[tid];
            unsigned seen = 0u;
            int d = 0;
            for (; d < 255; ++d) {
                const unsigned n = hist[tid][0][d];
                if (seen + n > k) break;
                seen += n;
            }
            prefix[tid] |= (unsigned)d << sh;
            left[tid] = k - seen;
        }
        __syncthreads();                // the scan has read the counts before the next digit zeroes them
    }

    // 2. thresholds
    const float fl = key_value(prefix[0]), pk = key_value(prefix[1]);
    const float r = __fsub_rn(pk, fl);
    const float on = __fadd_rn(fl, fmaxf(a.margin_db, __fmul_rn(a.onset, r)));
    const float off = __fadd_rn(fl, fmaxf(a.margin_db, __fmul_rn(a.offset, r)));
    if (tid == 0) {
        thr[0] = fl;
        thr[1] = pk;
        thr[2] = on;
        thr[3] = off;
    }

    // 3. decisive words: F / 64 + 1 of each kind, so that the word after the last frame (all silence) ends a run that reaches F
    const int W = F / 64 + 1;
    unsigned long long* sp = a.words + (f0 - a.frame_offsets[0]) / 64 + b;
    unsigned long long* si = sp + a.total_words;
    for (int w = wv; w < W; w += 16) {  // wave-uniform
        const int t = w * 64 + lane;
        const float v = t < F ? e[t] : 0.f;
        const unsigned long long s1 = __ballot(t < F && v >= on), s0 = __ballot(t >= F || v < off);
        if (lane == 0) {
            sp[w] = s1;
            si[w] = s0;
        }
    }
    __syncthreads();
    if (wv != 0) return;

    // 4. wave 0: hysteresis, runs, regions
    int32_t* regions = a.regions + 2 * (size_t)b * (size_t)a.cap;
    const bool writer = lane == 0;
    RunWalk walk;
    long long run_start = 0;
    unsigned long long carry = 0ull;    // the state of the frame before this step's first word, in every bit
    for (int base = 0; base < W; base += 64) {
        const int w = base + lane;
        unsigned long long g = w < W ? sp[w] : 0ull, p = w < W ? ~(g | si[w]) : 0ull;
        scan64(g, p);                   // the word's states if silence came in; p: the bits that take what comes in
        unsigned long long G = __ballot(g >> 63), P = __ballot(p >> 63);
        scan64(G, P);                   // bit l: the state after lane l's word, if silence came into the step
        const unsigned long long after = G | (P & carry);
        const unsigned long long in = lane ? 0ull - ((after >> (lane ? lane - 1 : 0)) & 1ull) : carry;
        const unsigned long long x = g | (p & in);
        const unsigned long long edges = x ^ (x << 1 | (in & 1ull));
        carry = 0ull - (after >> 63);
        unsigned long long busy = __ballot(edges != 0ull);
        while (busy) {                  // the words with a run start or end, in order; every lane walks the same edges
            const int l = __builtin_ctzll(busy);
            busy &= busy - 1ull;
            unsigned long long ed = shfl64(edges, l);
            const unsigned long long xs = shfl64(x, l);
            const long long t0 = (long long)(base + l) * 64;
            while (ed) {
                const int bit = __builtin_ctzll(ed);
                ed &= ed - 1ull;
                if ((xs >> bit) & 1ull) run_start = t0 + bit;
                else walk.run(a, F, regions, writer, run_start, t0 + bit);
            }
        }
    }
    walk.close(a, F, regions, writer);
    walk.emit(a, regions, writer);
    if (writer) a.counts[b] = walk.count;
}

size_t words_of_a_kind(long long total_frames, int B) { return (size_t)(total_frames / 64) + (size_t)B + 1; }

}  // namespace

extern "C" {

int vp_vad_num_frames(long long n, int win, int hop) {
    if (win < 1 || hop < 1 || n < 0) return 0;
    const long long f = n < win ? 0 : 1 + (n - win) / hop;
    return f > 0x7fffffffLL ? 0x7fffffff : (int)f;
}

int vp_vad_frame_db_f32(vp_ctx* ctx, const float* wave, const int32_t* offsets, const int32_t* frame_offsets, int B, int win, int hop,
                        float preemph, float* e, vp_stream stream) {
    if (B < 1 || B > MAX_B || hop < 1 || win < hop || win > MAX_WIN || !(preemph >= 0.f && preemph < 1.f))
        VP_FAIL(ctx, VP_EINVAL, "vad_frame_db: 1 <= B <= %d, 1 <= hop <= win <= %d, 0 <= preemph < 1", MAX_B, MAX_WIN);
    if (!ctx || !wave || !offsets || !frame_offsets || !e) VP_FAIL(ctx, VP_EINVAL, "vad_frame_db: null pointer");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> off, foff;
    int rc = read_offsets(ctx, offsets, B, off, st);
    if (rc == VP_OK) rc = read_offsets(ctx, frame_offsets, B, foff, st);
    if (rc == VP_EINVAL) VP_FAIL(ctx, VP_EINVAL, "vad_frame_db: offsets must start at >= 0 and not decrease");
    if (rc != VP_OK) return rc;
    int most = 0;
    for (int b = 0; b < B; ++b) {
        const int F = num_frames((long long)off[b + 1] - off[b], win, hop);
        if (foff[b + 1] - foff[b] != F)
            VP_FAIL(ctx, VP_EINVAL, "vad_frame_db: frame_offsets of recording %d span %d frames, vp_vad_num_frames gives %d", b,
                    foff[b + 1] - foff[b], F);
        most = F > most ? F : most;
    }
    if (most == 0) return VP_OK;
    FrameArgs a{};
    a.wave = wave;
    a.offsets = offsets;
    a.frame_offsets = frame_offsets;
    a.win = win;
    a.hop = hop;
    const int fit = 1 + (TILE_FLOATS - win) / hop;          // (fit - 1) hop + win <= TILE_FLOATS
    a.tile_frames = fit < TILE_FRAMES ? fit : TILE_FRAMES;
    a.preemph = preemph;
    a.e = e;
    const int tiles = (most + a.tile_frames - 1) / a.tile_frames;
    hipLaunchKernelGGL(frame_db_kernel, dim3(tiles < 65535 ? tiles : 65535, B), dim3(256), 0, st, a);
    VP_LAUNCH_CHECK(ctx, "frame_db_kernel");
    return VP_OK;
}

size_t vp_vad_workspace_bytes(long long total_frames, int B) {
    if (total_frames < 0 || B < 1) return 0;
    return 2 * words_of_a_kind(total_frames, B) * 8;
}

int vp_vad_regions_f32(vp_ctx* ctx, const float* e, const int32_t* frame_offsets, int B, float floor_pct, float peak_pct,
                       float margin_db, float onset, float offset, int min_gap, int min_speech, int pad, float* thr, int32_t* counts,
                       int32_t* regions, int cap, void* ws, size_t ws_bytes, vp_stream stream) {
    if (B < 1 || B > MAX_B || !(floor_pct >= 0.f && floor_pct <= peak_pct && peak_pct <= 1.f) ||
        !(offset >= 0.f && offset <= onset && onset <= 1.f) || !(margin_db >= 0.f) || min_gap < 1 || min_speech < 1 || pad < 0 || cap < 0)
        VP_FAIL(ctx, VP_EINVAL, "vad_regions: 1 <= B <= %d, 0 <= floor_pct <= peak_pct <= 1, 0 <= offset <= onset <= 1, margin_db >= 0, "
                                "min_gap, min_speech >= 1, pad, cap >= 0", MAX_B);
    if (!ctx || !e || !frame_offsets || !thr || !counts || !regions || !ws) VP_FAIL(ctx, VP_EINVAL, "vad_regions: null pointer");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> foff;
    const int rc = read_offsets(ctx, frame_offsets, B, foff, st);
    if (rc == VP_EINVAL) VP_FAIL(ctx, VP_EINVAL, "vad_regions: frame_offsets must start at >= 0 and not decrease");
    if (rc != VP_OK) return rc;
    const long long total = (long long)foff[B] - foff[0];
    const size_t need = vp_vad_workspace_bytes(total, B);
    if (ws_bytes < need) VP_FAIL(ctx, VP_EWORKSPACE, "vad_regions: workspace %zu < %zu bytes", ws_bytes, need);
    RegionArgs a{};
    a.e = e;
    a.frame_offsets = frame_offsets;
    a.floor_pct = floor_pct;
    a.peak_pct = peak_pct;
    a.margin_db = margin_db;
    a.onset = onset;
    a.offset = offset;
    a.min_gap = min_gap;
    a.min_speech = min_speech;
    a.pad = pad;
    a.cap = cap;
    a.thr = thr;
    a.counts = counts;
    a.regions = regions;
    a.words = (unsigned long long*)ws;
    a.total_words = (long long)words_of_a_kind(total, B);
    hipLaunchKernelGGL(regions_kernel, dim3(B), dim3(1024), 0, st, a);
    VP_LAUNCH_CHECK(ctx, "regions_kernel");
    return VP_OK;
}

}  // extern "C"
