// The kernels at both ends of a sampler step on gfx950, fp32, one thread per latent element: "assemble the UNet input and latch the
// counter", "CFG-combine eps and apply the DDIM, inversion, PLMS or DPM-Solver++ update", "re-noise the given latents", and between the two
// ends "turn a v-model's output into eps" and "rescale the guided output to the conditional row's std" (the one reduction here).
// Every form of a step -- host index, device counter, seeded, over slots -- runs ONE device body per idea (cfg_eps_at, step_update,
// invert_update, plms_update, dpm_update, eps_from_v, the rescale pair, known_blend_at), so an element gets the same bits from each.
#include "seer_common.h"
#include "seer_philox.h"
#include <cstdint>
#include <initializer_list>

namespace {

// ---- the update bodies --------------------------------------------------------------------------------------------------------------
// the CFG-combined eps of latent element i of [b, C, Ft - cond_f, HW]: eps is [2b (uc then c) or b, C, Ft, HW], frames >= cond_f
__device__ __forceinline__ float cfg_eps_at(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW,
                                            float scale, int64_t i) {
    const int Fp = Ft - cond_f;
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % Fp);
    const int c = (int)((i / ((int64_t)HW * Fp)) % C);
    const int bi = (int)(i / ((int64_t)HW * Fp * C));
    const int64_t eoff = (((int64_t)bi * C + c) * Ft + (f + cond_f)) * HW + hw;
    if (!cfg) return eps[eoff];
    const float eu = eps[eoff];
    const float ec = eps[eoff + (int64_t)b * C * Ft * HW];
    return eu + scale * (ec - eu);
}

// where the sigma term of a DDIM update comes from: tensor[i], or -- seed != nullptr -- temperature times normal `el` of Philox stream
// 1 of the clip's seed at the schedule index (seer_philox.h), drawn here instead of read, so a captured step has nothing to draw
// between its launches and a clip's noise does not depend on its batch row or slot.  Neither: no noise (eta = 0).
struct StepNoise {
    const float* tensor;
    const uint32_t* seed;
    float temperature;
    uint32_t el;
};

// DDIM_TERM: x_prev = ... + nz, with nz = 0.f where there is no noise (the DDIM kernels always add).  NO_TERM: the PLMS update has no
// such add, and x + 0.f is not an identity on a zero's sign, so the two are told apart at compile time.
enum NoiseTerm { NO_TERM, DDIM_TERM };

// the update of element i from e' (the CFG-combined eps, multistep-combined for PLMS) and row `index` of coef = (a_t, a_prev, sigma,
// sqrt(1 - a_t)).  The sigma term is sigma * noise[i] or sigma * (temperature * n), rounded fp32 products, then the add; sigma == 0
// (uniform over a clip's threads) draws nothing and gives the bits of no noise.  x may alias x_prev: the element is read before it
// is written.
template <NoiseTerm TERM>
__device__ __forceinline__ void step_update(float ep, const float* __restrict__ coef, int index, const float* x, StepNoise noise,
                                            float* x_prev, float* __restrict__ pred_x0, int64_t i) {
    const float a_t = coef[4 * index], a_prev = coef[4 * index + 1], sigma = coef[4 * index + 2], s1m = coef[4 * index + 3];
    const float xv = x[i];
    const float x0 = (xv - s1m * ep) / sqrtf(a_t);
    const float dir = sqrtf(1.f - a_prev - sigma * sigma) * ep;
    if constexpr (TERM == DDIM_TERM) {
        float nz = 0.f;
        if (noise.seed) {
            if (sigma != 0.f) {
                const float tn = noise.temperature * seer_philox::normal_at(noise.seed[0], noise.seed[1], seer_philox::STREAM_STEP,
                                                                            (uint32_t)index, noise.el);
                nz = sigma * tn;
            }
        } else if (noise.tensor) {
            nz = sigma * noise.tensor[i];
        }
        x_prev[i] = sqrtf(a_prev) * x0 + dir + nz;
    } else {
        x_prev[i] = sqrtf(a_prev) * x0 + dir;
    }
    if (pred_x0) pred_x0[i] = x0;
}

// DDIM inversion (CompVis ddim.py encode(), eta = 0 by definition): the probability-flow ODE one step UPWARD.  x is the latent at the
// level of a_prev, e the CFG-combined eps the model gave at the timestep of a_t; x_next is the latent at the level of a_t.  sigma is
// not read.  x may alias x_next: the element is read before it is written.
__device__ __forceinline__ void invert_update(float e, const float* __restrict__ coef, int index, const float* x, float* x_next,
                                              float* __restrict__ pred_x0, int64_t i) {
    const float a_t = coef[4 * index], a_prev = coef[4 * index + 1], s1m = coef[4 * index + 3];
    const float xv = x[i];
    const float x0 = (xv - sqrtf(1.f - a_prev) * e) / sqrtf(a_prev);
    x_next[i] = sqrtf(a_t) * x0 + s1m * e;
    if (pred_x0) pred_x0[i] = x0;
}

// CFG + PLMS update (ldm/models/diffusion/plms.py:199-236, eta = 0).  e = the CFG-combined eps of this evaluation; h1, h2, h3 =
// earlier e, newest first.  e' by order:
//   0: e (the first step's provisional DDIM update)   1: (h1 + e)/2 (the first step's final update: h1 = first evaluation, e = second)
//   2: (3e - h1)/2   3: (23e - 16h1 + 5h2)/12   4: (55e - 59h1 + 37h2 - 9h3)/24
// then step_update with e'.  A history term the order does not use is never read (stale slots may hold NaN, and 0 * NaN is NaN).
// e_out (may alias a history slot: every thread reads its element before it writes it) receives e, not e' (plms.py:160), for every
// order but 1, whose e is the second evaluation that plms.py does not keep.
__device__ __forceinline__ void plms_update(float e, int order, const float* h1, const float* h2, const float* h3, int64_t i,
                                            const float* __restrict__ coef, int index, const float* x, float* x_prev,
                                            float* __restrict__ pred_x0, float* e_out) {
    float ep;
    switch (order) {
        case 0: ep = e; break;
        case 1: ep = (h1[i] + e) / 2.f; break;
        case 2: ep = (3.f * e - h1[i]) / 2.f; break;
        case 3: ep = (23.f * e - 16.f * h1[i] + 5.f * h2[i]) / 12.f; break;
        default: ep = (55.f * e - 59.f * h1[i] + 37.f * h2[i] - 9.f * h3[i]) / 24.f; break;
    }
    step_update<NO_TERM>(ep, coef, index, x, StepNoise{}, x_prev, pred_x0, i);
    if (e_out && order != 1) e_out[i] = e;
}

// CFG + DPM-Solver++ update (first order, or second order multistep "2M"; eta = 0).  e = the CFG-combined eps; row = the schedule
// entry's six words of the DPM table (include/seer_hip.h, seer_cfg_dpm_step): (sigma_s, 1/alpha_s, c_x, c_D1, c_D2, c_Dprev), every
// exp and log of the exponential integrator folded into them on the host.  D = (x - sigma_s e) / alpha_s is the data prediction;
//   order 1: x_prev = c_x x + c_D1 D                      order 2: x_prev = c_x x + c_D2 D + c_Dprev d_prev[i]
// d_prev (the D of the step before) is read at order 2 only: at order 1 it may be NULL or hold anything, NaN included.  x may alias
// x_prev and d_prev may alias pred_x0, which receives D: every thread reads its element of each before it writes it.
enum { DPM_ROW_WORDS = 6 };

__device__ __forceinline__ void dpm_update(float e, const float* __restrict__ row, int order, const float* x, const float* d_prev,
                                           float* x_prev, float* pred_x0, int64_t i) {
    const float xv = x[i];
    const float d = (xv - row[0] * e) * row[1];
    if (order == 2) {
        const float dp = d_prev[i];
        x_prev[i] = row[2] * xv + row[4] * d + row[5] * dp;
    } else {
        x_prev[i] = row[2] * xv + row[3] * d;
    }
    if (pred_x0) pred_x0[i] = d;
}

// A v-prediction model's output as eps (diffusers get_velocity read backwards): with x_t = sqrt(a) x0 + sqrt(1 - a) eps the model gives
// v = sqrt(a) eps - sqrt(1 - a) x0, so eps = sqrt(a) v + sqrt(1 - a) x_t.  a_t and s1m are words 0 and 3 of the DDIM coefficient row of the
// timestep the model was evaluated at.  Affine in v with the same x for both rows of a CFG pair: converting the rows and CFG-combining
// them after gives the eps of combining first, so the conversion sits in front of the update kernels and those do not know of it.
__device__ __forceinline__ float eps_from_v(float v, float x, float a_t, float s1m) { return sqrtf(a_t) * v + s1m * x; }

// element i of out / v [rows, C, Ft - cond_f predicted frames of Ft, HW], counted over the predicted frames only: the conditioning
// frames of the model output are neither read nor written.  xrow = the latent row [C, Ft - cond_f, HW] this output row was evaluated
// at, `per` = its element count, e = i's offset in it.  out may alias v: the element is read before it is written.
__device__ __forceinline__ void v_to_eps_at(const float* v, const float* __restrict__ xrow, const float* __restrict__ row, int C,
                                            int Ft, int cond_f, int HW, int64_t r, int64_t e, float* out) {
    const int Fp = Ft - cond_f;
    const int hw = (int)(e % HW);
    const int f = (int)((e / HW) % Fp);
    const int c = (int)(e / ((int64_t)HW * Fp));
    const int64_t off = ((r * C + c) * Ft + (f + cond_f)) * HW + hw;
    out[off] = eps_from_v(v[off], xrow[e], row[0], row[3]);
}

// ---- one clip batch: the schedule index from the host, or in DEVICE memory (a whole p_sample_ddim captured in one hipGraph: the
// kernel arguments of a replay are frozen, the step counter is not).  step[0] = index of the NEXT step to run, step[1] = index of the
// step in flight.  seer_ddim_step_begin (first kernel of a step) reads step[0] everywhere and one thread copies it to step[1]; the
// update (last kernel) reads step[1] everywhere and one thread writes step[0] = index - 1: no kernel both reads and writes a word, so
// a chain of replays walks the schedule downwards without the host touching device memory.
// Input assembly of ddim_video.py:189,201-203: the UNet input [reps*b, C, F, HW] = cat([x0_emb, x], frames), repeated for the CFG
// pair, and t[reps*b] = timesteps[index].
__global__ void ddim_assemble_kernel(const float* __restrict__ x0_emb, const float* __restrict__ x, int b, int reps, int C, int f1,
                                     int Fp, int HW, const int64_t* __restrict__ t_table, int* __restrict__ step,
                                     float* __restrict__ sample, int64_t* __restrict__ t_out) {
    const int F = f1 + Fp;
    const int64_t per = (int64_t)b * C * F * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int index = step[0];
    if (i == 0) step[1] = index;
    if (i < reps * b) t_out[i] = t_table[index];
    if (i >= per) return;
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int64_t bc = i / ((int64_t)HW * F);            // bi * C + c
    const float v = f < f1 ? x0_emb[(bc * f1 + f) * HW + hw] : x[(bc * Fp + (f - f1)) * HW + hw];
    for (int r = 0; r < reps; ++r) sample[i + r * per] = v;
}

// step == nullptr: the host's `index`; else index = step[1] and one thread writes step[0] = index - 1; a counter that ran past the
// schedule's end (index < 0) reads no coefficient row and writes no element.  The noise is `noise`, or -- seeds uint32 [b][2] (lo, hi),
// one pair per batch row -- seeded with `temperature`, or absent.  x may alias x_prev.
__global__ void cfg_ddim_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                const float* __restrict__ coef, int index, int* __restrict__ step, const float* x,
                                const float* __restrict__ noise, const uint32_t* __restrict__ seeds, float temperature, float* x_prev,
                                float* __restrict__ pred_x0) {
    const int64_t per_clip = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) {
        index = step[1];
        if (i == 0) step[0] = index - 1;
    }
    if (index < 0 || i >= (int64_t)b * per_clip) return;
    const int64_t bi = i / per_clip;
    step_update<DDIM_TERM>(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), coef, index, x,
                           StepNoise{noise, seeds ? seeds + 2 * bi : nullptr, temperature, (uint32_t)(i - bi * per_clip)}, x_prev,
                           pred_x0, i);
}

// The conversion in front of an update kernel, for a model that predicts v: v [reps * b (uc rows then c rows, or b), C, Ft, HW] -> eps in
// the same layout, frames >= cond_f only; output row r was evaluated at x[r mod b].  step == nullptr: the host's `index`; else index =
// step[1], which seer_ddim_step_begin latched -- it is only read, NO counter word is written here: the kernel sits between the begin
// kernel and the update kernel, and the update still finds step[1] as begin left it.  An index outside 0 .. nsched - 1 reads no row and
// writes no element.  out may alias v.
__global__ void v_to_eps_kernel(const float* v, int reps, int b, int C, int Ft, int cond_f, int HW, const float* __restrict__ coef,
                                int nsched, int index, const int* __restrict__ step, const float* __restrict__ x, float* out) {
    const int64_t per = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) index = step[1];
    if (index < 0 || index >= nsched || i >= (int64_t)reps * b * per) return;
    const int64_t r = i / per;
    v_to_eps_at(v, x + (r % b) * per, coef + 4 * index, C, Ft, cond_f, HW, r, i - r * per, out);
}

// The inversion step.  step == nullptr: the host's `index`; else index = step[1], one thread writes step[0] = index + 1 (the chain
// walks the schedule UPWARDS), and `limit` (one word in device memory: a replay's arguments are frozen, and the rows of a static table
// beyond the schedule hold a_prev = 0, which this update divides by) ends it: index < 0 or index >= limit[0] reads no coefficient
// row and writes no element.  x may alias x_next.
__global__ void cfg_ddim_invert_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                       const float* __restrict__ coef, int index, int* __restrict__ step,
                                       const int* __restrict__ limit, const float* x, float* x_next, float* __restrict__ pred_x0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) {
        index = step[1];
        if (i == 0) step[0] = index + 1;
        if (index < 0 || index >= limit[0]) return;
    }
    if (i >= (int64_t)b * C * (Ft - cond_f) * HW) return;
    invert_update(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), coef, index, x, x_next, pred_x0, i);
}

__global__ void cfg_plms_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                const float* __restrict__ coef, int index, int order, const float* x, const float* h1,
                                const float* h2, const float* h3, float* x_prev, float* __restrict__ pred_x0, float* e_out) {
    const int64_t n = (int64_t)b * C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    plms_update(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), order, h1, h2, h3, i, coef, index, x, x_prev, pred_x0,
                e_out);
}

// The captured form: the index is step[1] (seer_ddim_step_begin copied it there) and the history is a 3-slot ring of [n] fp32
// slots.  ring_state int32[4] holds (valid, newest) twice, by parity of the index: a step reads pair (index & 1) and one thread
// writes pair ((index - 1) & 1) = (min(valid + 1, 3), slot) with slot = (newest + 1) % 3, the slot this step stores e into (the
// oldest one once all three are valid); it also writes step[0] = index - 1.  No kernel reads and writes the same word.
// valid = 0 is a plain DDIM step (order 0), valid = k > 0 is order k + 1.  index < 0: those words are written all the same, but no
// coefficient row is read and no element of x_prev, pred_x0 or the ring written.
__global__ void cfg_plms_dev_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                    const float* __restrict__ coef, int* __restrict__ step, float* ring,
                                    int* __restrict__ ring_state, const float* x, float* x_prev, float* __restrict__ pred_x0) {
    const int64_t n = (int64_t)b * C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int index = step[1];
    const int* rs = ring_state + 2 * (index & 1);
    int valid = rs[0], newest = rs[1];
    if (valid < 0 || valid > 3 || newest < 0 || newest > 2) valid = 0, newest = 2;     // never index outside the ring
    const int slot = newest == 2 ? 0 : newest + 1;
    if (i == 0) {
        step[0] = index - 1;
        int* ws = ring_state + 2 * ((index - 1) & 1);
        ws[0] = valid < 3 ? valid + 1 : 3;
        ws[1] = slot;
    }
    if (index < 0 || i >= n) return;
    const float* h1 = ring + (int64_t)newest * n;
    const float* h2 = ring + (int64_t)(newest == 0 ? 2 : newest - 1) * n;
    const float* h3 = ring + (int64_t)slot * n;
    plms_update(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), valid == 0 ? 0 : valid + 1, h1, h2, h3, i, coef, index,
                x, x_prev, pred_x0, ring + (int64_t)slot * n);
}

// The DPM-Solver++ step.  step == nullptr: the host's `index` and `order`.  Else the captured form: index = step[1], and the order comes
// from state int32[4] = (history valid for an even index, for an odd one, the sampler's order, whether a schedule's final step is first
// order): order 2 when the word of the index's parity is 1, state[2] is 2 and not (index == 0 and state[3] != 0), else order 1.  One
// thread writes step[0] = index - 1 and the valid word of parity (index - 1): 1 when this launch stores a D, 0 when it does not.
// state[2] and state[3] are only read: no kernel reads and writes the same word.  The history is pred_x0 itself (d_prev == pred_x0 in
// that form).  An index outside 0 .. nsched - 1 reads no table row and writes no element.
__global__ void cfg_dpm_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                               const float* __restrict__ coef, int nsched, int index, int order, int* __restrict__ step,
                               int* __restrict__ state, const float* x, const float* d_prev, float* x_prev, float* pred_x0) {
    const int64_t n = (int64_t)b * C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) {
        index = step[1];
        const bool in_table = index >= 0 && index < nsched;
        order = state[index & 1] == 1 && state[2] == 2 && !(index == 0 && state[3] != 0) ? 2 : 1;
        if (i == 0) {
            step[0] = index - 1;
            state[(index - 1) & 1] = in_table ? 1 : 0;
        }
    }
    if (index < 0 || index >= nsched || i >= n) return;
    dpm_update(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), coef + DPM_ROW_WORDS * index, order, x, d_prev, x_prev, pred_x0,
               i);
}

// ---- the captured step over SLOTS (continuous batching, seervideoldm_amd/slots.py): per-slot forms of ddim_assemble_kernel and
// cfg_ddim_kernel.  Slot s owns rows s and slots + s of the [uc | c] pair, its own schedule tables t_table[s][nsched] and
// coef[s][nsched][4], its own guidance scale scale[s] and its own counter pair step[s][0..1].  An idle slot (index < 0) still gets
// finite input rows (the host zeroed its latents; its t is row 0 of its table) and its update writes nothing.  As above, no kernel
// reads and writes the same word.  The int64 tables move as int32 pairs: no pointer is relied on beyond 4-byte alignment.
//
// With a SAMPLER per slot, DDIM and PLMS clips run side by side.  state int32 [slots][8] = (phase, valid, newest, -) of the NEXT
// step, then the same three words of the step IN FLIGHT; ring fp32 [slots][3][C*Fp*HW] = the slot's earlier e, x_prov
// [slots][C*Fp*HW] its provisional latent.  The begin kernel reads next words and writes in-flight words, the update kernel reads
// in-flight words and writes next words.  Phases (plms.py:145-160):
//   0  DDIM, for the whole clip           1  PLMS first step, first evaluation: x_prov = order 0 of x, e -> ring slot 0
//   2  PLMS first step, second evaluation at x_prov and the NEXT timestep: order 1 on x      3  PLMS later steps: order valid + 1
// A phase outside 0..3 is read as 0; in phase 3 a (valid, newest) outside 0..3 x 0..2 is read as (0, 2), as cfg_plms_dev_kernel does.
enum { SLOT_STATE_WORDS = 8, SLOT_IN_FLIGHT = 4 };

// state == nullptr (seer_slot_step_begin): every slot is in phase 0 and x_prov is not read
__global__ void slot_assemble_kernel(const float* __restrict__ x0_emb, const float* __restrict__ x,
                                     const float* __restrict__ x_prov, int slots, int reps, int C, int f1, int Fp, int HW,
                                     const int* __restrict__ t_table, int nsched, int* __restrict__ step, int* __restrict__ state,
                                     float* __restrict__ sample, int* __restrict__ t_out) {
    const int F = f1 + Fp;
    const int64_t per_slot = (int64_t)C * F * HW;
    const int64_t per = (int64_t)slots * per_slot;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    const int s = (int)(i / per_slot);
    int* const next = state ? state + SLOT_STATE_WORDS * s : nullptr;
    const int phase = next ? next[0] : 0;
    if (i == (int64_t)s * per_slot) {                    // the slot's first element: its counter, its state and its timesteps
        int index = step[2 * s];
        step[2 * s + 1] = index;
        if (next) {
            int* fly = next + SLOT_IN_FLIGHT;
            fly[0] = phase, fly[1] = next[1], fly[2] = next[2];
        }
        if (phase == 2) --index;                         // the second evaluation runs at t_next = t_table[max(index - 1, 0)]
        const int row = index < 0 ? 0 : (index < nsched ? index : nsched - 1);      // never outside the table
        const int* t = t_table + 2 * ((int64_t)s * nsched + row);
        for (int r = 0; r < reps; ++r) {
            t_out[2 * (r * slots + s)] = t[0];
            t_out[2 * (r * slots + s) + 1] = t[1];
        }
    }
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int64_t bc = i / ((int64_t)HW * F);            // s * C + c
    const float* lat = phase == 2 ? x_prov : x;
    const float v = f < f1 ? x0_emb[(bc * f1 + f) * HW + hw] : lat[(bc * Fp + (f - f1)) * HW + hw];
    for (int r = 0; r < reps; ++r) sample[i + r * per] = v;
}

// CFG always on: cfg_eps_at with scale[s], step_update with row step[s][1] of coef[s].  seeds == nullptr: eta = 0, no noise term;
// else a seed pair and a temperature per slot, sigma being column 2 of the slot's own coef rows.  x may alias x_prev.
__global__ void slot_cfg_ddim_kernel(const float* __restrict__ eps, int slots, int C, int Ft, int cond_f, int HW,
                                     const float* __restrict__ scale, const float* __restrict__ coef, int nsched,
                                     int* __restrict__ step, const float* x, const uint32_t* __restrict__ seeds,
                                     const float* __restrict__ temperature, float* x_prev, float* __restrict__ pred_x0) {
    const int64_t per_slot = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int s = (int)(i / per_slot);
    const int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;            // idle (or a counter outside the table): nothing of this slot is written
    if (i == (int64_t)s * per_slot) step[2 * s] = index - 1;
    StepNoise noise{};
    if (seeds) noise = StepNoise{nullptr, seeds + 2 * s, temperature[s], (uint32_t)(i - (int64_t)s * per_slot)};
    step_update<DDIM_TERM>(cfg_eps_at(eps, 1, slots, C, Ft, cond_f, HW, scale[s], i), coef + (int64_t)s * nsched * 4, index, x, noise,
                           x_prev, pred_x0, i);
}

// CFG always on, eta = 0.  The arithmetic is cfg_eps_at with scale[s], then step_update (phase 0) or plms_update (phases 1 to 3)
// with row step[s][1] of coef[s]: an element gets the bits of seer_cfg_ddim_step / seer_cfg_plms_step.  x may alias x_prev.
__global__ void slot_cfg_plms_kernel(const float* __restrict__ eps, int slots, int C, int Ft, int cond_f, int HW,
                                     const float* __restrict__ scale, const float* __restrict__ coef, int nsched,
                                     int* __restrict__ step, int* __restrict__ state, float* ring, const float* x, float* x_prov,
                                     float* x_prev, float* __restrict__ pred_x0) {
    const int64_t per_slot = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int s = (int)(i / per_slot);
    const int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;            // idle (or a counter outside the table): nothing of this slot is written
    const int* fly = state + SLOT_STATE_WORDS * s + SLOT_IN_FLIGHT;
    int* next = state + SLOT_STATE_WORDS * s;
    const bool first = i == (int64_t)s * per_slot;
    const float* cf = coef + (int64_t)s * nsched * 4;
    const float e = cfg_eps_at(eps, 1, slots, C, Ft, cond_f, HW, scale[s], i);
    // entry k of the slot's ring, based so that [i] (an index over all slots) is this element: (3 s + k) per_slot + (i - s per_slot)
    float* const rs = ring + 2 * (int64_t)s * per_slot;
    const int phase = fly[0];
    if (phase == 1) {
        if (first) next[0] = 2, next[1] = 1, next[2] = 0;
        plms_update(e, 0, nullptr, nullptr, nullptr, i, cf, index, x, x_prov, nullptr, rs);
    } else if (phase == 2) {
        int newest = fly[2];
        if (newest < 0 || newest > 2) newest = 0;        // never index outside the ring
        if (first) step[2 * s] = index - 1, next[0] = 3;
        plms_update(e, 1, rs + newest * per_slot, nullptr, nullptr, i, cf, index, x, x_prev, pred_x0, nullptr);
    } else if (phase == 3) {
        int valid = fly[1], newest = fly[2];
        if (valid < 0 || valid > 3 || newest < 0 || newest > 2) valid = 0, newest = 2;
        const int slot = newest == 2 ? 0 : newest + 1;
        if (first) step[2 * s] = index - 1, next[1] = valid < 3 ? valid + 1 : 3, next[2] = slot;
        plms_update(e, valid == 0 ? 0 : valid + 1, rs + newest * per_slot, rs + (newest == 0 ? 2 : newest - 1) * per_slot,
                    rs + slot * per_slot, i, cf, index, x, x_prev, pred_x0, rs + slot * per_slot);
    } else {
        if (first) step[2 * s] = index - 1;
        step_update<DDIM_TERM>(e, cf, index, x, StepNoise{}, x_prev, pred_x0, i);
    }
}

// DDIM and DPM-Solver++ clips side by side.  CFG always on, eta = 0.  dpm_coef [slots][nsched][6] holds a DPM table per slot, state
// int32 [slots][4] the four words of cfg_dpm_kernel per slot, with word 2 = the slot's sampler: 0 DDIM, 1 DPM first order, 2 2M (any
// other value is read as 0).  The arithmetic is cfg_eps_at with scale[s], then step_update (a DDIM slot, as slot_cfg_ddim_kernel
// without seeds) or dpm_update with cfg_dpm_kernel's order rule: an element gets the bits of seer_cfg_ddim_step / seer_cfg_dpm_step.
// d_hist is the slot's pred_x0 rows: an order-2 step reads the D of the step before from it, every step writes its own over it.
// A DPM slot's first thread also writes the valid word of parity (index - 1); words 2 and 3 are only read.  x may alias x_prev.
__global__ void slot_cfg_dpm_kernel(const float* __restrict__ eps, int slots, int C, int Ft, int cond_f, int HW,
                                    const float* __restrict__ scale, const float* __restrict__ coef,
                                    const float* __restrict__ dpm_coef, int nsched, int* __restrict__ step, int* __restrict__ state,
                                    const float* x, float* x_prev, float* d_hist) {
    const int64_t per_slot = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int s = (int)(i / per_slot);
    const int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;            // idle (or a counter outside the table): nothing of this slot is written
    int* st = state + 4 * s;
    const int sampler = st[2];
    const bool first = i == (int64_t)s * per_slot;
    const float e = cfg_eps_at(eps, 1, slots, C, Ft, cond_f, HW, scale[s], i);
    if (sampler == 1 || sampler == 2) {
        const int order = st[index & 1] == 1 && sampler == 2 && !(index == 0 && st[3] != 0) ? 2 : 1;
        if (first) step[2 * s] = index - 1, st[(index - 1) & 1] = 1;
        dpm_update(e, dpm_coef + ((int64_t)s * nsched + index) * DPM_ROW_WORDS, order, x, d_hist, x_prev, d_hist, i);
    } else {
        if (first) step[2 * s] = index - 1;
        step_update<DDIM_TERM>(e, coef + (int64_t)s * nsched * 4, index, x, StepNoise{}, x_prev, d_hist, i);
    }
}

// v_to_eps_kernel over slots, between a slot begin kernel and a slot update kernel: rows s and slots + s of the [uc | c] pair are slot
// s, converted with row step[s][1] of coef[s] against x[s].  state != nullptr (a queue with a sampler per slot, slots.py plms=True): the
// slot's IN-FLIGHT phase word, as slot_assemble_kernel reads the next one; in phase 2 that kernel assembled x_prov[s] at
// t_table[max(index - 1, 0)], so the conversion reads x_prov[s] and that row.  An idle slot, or a counter outside the table, leaves its
// rows untouched; no step or state word is written.  out may alias v.
__global__ void slot_v_to_eps_kernel(const float* v, int slots, int C, int Ft, int cond_f, int HW, const float* __restrict__ coef,
                                     int nsched, const int* __restrict__ step, const int* __restrict__ state,
                                     const float* __restrict__ x, const float* __restrict__ x_prov, float* out) {
    const int64_t per = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * (int64_t)slots * per) return;
    const int64_t r = i / per;
    const int s = (int)(r % slots);
    int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;
    const float* lat = x;
    if (state && state[SLOT_STATE_WORDS * s + SLOT_IN_FLIGHT] == 2) {
        lat = x_prov;
        index = index > 0 ? index - 1 : 0;
    }
    v_to_eps_at(v, lat + s * per, coef + ((int64_t)s * nsched + index) * 4, C, Ft, cond_f, HW, r, i - r * per, out);
}

// ---- guidance rescale (Lin et al. 2023, section 3.4; diffusers rescale_noise_cfg): the guided output g of a clip, scaled so that its std
// over the clip's predicted frames matches the conditional row's, blended with the unscaled g by phi -- out = m g with
//   m = phi sqrt(q_c / q_g) + (1 - phi),   q = n S2 - S1^2 (n^2 times the variance: the n - 1 of an unbiased std cancels in the ratio),
// written to BOTH rows of the clip's [uc | c] pair: the update kernel behind it then combines eu == ec, which gives ec again exactly
// (ec - eu = +0, scale * 0 = 0, eu + 0 = eu, contracted or not), so no update kernel knows of it.  It is the first thing here that needs
// a whole clip, and it is two launches over the same grid (P tiles of SEER_RESCALE_TILE elements, clips): "moments" reduces a tile to
// four doubles (sum c, sum c^2, sum g, sum g^2) in a fixed order -- per thread in index order, __shfl_xor across the wave, the waves
// through LDS in wave order -- and STORES them to ws[clip][p][4]; "apply" sums a clip's P partials in index order, makes m and writes
// m g over the tile.  No atomics, no counter, no waiting inside a launch: a clip's m has the same bits in every run, and, because the
// tiling follows from n alone, for every batch size, row and slot.  g is cfg_eps_at's value in both passes: the moments are taken of
// exactly the numbers that get scaled.
// The form is read from the pointers: scale_v == nullptr is the solo form (`scale`, `phi` for every clip); else slot s uses scale_v[s]
// and phi_v[s], and a slot that is idle (step[s][1] outside 0 .. nsched - 1) or has phi_v[s] == 0 has no word written by either kernel.
enum { RESCALE_THREADS = 256, RESCALE_PER_THREAD = SEER_RESCALE_TILE / RESCALE_THREADS };
static_assert(SEER_RESCALE_TILE % RESCALE_THREADS == 0 && RESCALE_PER_THREAD >= 1, "SEER_RESCALE_TILE is a multiple of 256");

struct RescaleClip {
    bool active;
    float scale, phi;
};

__device__ __forceinline__ RescaleClip rescale_clip(int clip, float scale, float phi, const float* __restrict__ scale_v,
                                                    const float* __restrict__ phi_v, int nsched, const int* __restrict__ step) {
    if (!scale_v) return RescaleClip{true, scale, phi};
    const int index = step[2 * clip + 1];
    const float ph = phi_v[clip];
    return RescaleClip{index >= 0 && index < nsched && ph != 0.f, scale_v[clip], ph};
}

// the offset in eps [2 rows, C, Ft, HW] of element e (counted over the predicted frames) of the uc row of `clip`; its c row is
// rows * C * Ft * HW further on (cfg_eps_at's own addressing)
__device__ __forceinline__ int64_t rescale_offset(int clip, int C, int Ft, int cond_f, int HW, int64_t e) {
    const int Fp = Ft - cond_f;
    const int hw = (int)(e % HW);
    const int f = (int)((e / HW) % Fp);
    const int c = (int)(e / ((int64_t)HW * Fp));
    return (((int64_t)clip * C + c) * Ft + (f + cond_f)) * HW + hw;
}

__global__ __launch_bounds__(RESCALE_THREADS) void cfg_rescale_moments_kernel(
    const float* __restrict__ eps, int rows, int C, int Ft, int cond_f, int HW, float scale, float phi,
    const float* __restrict__ scale_v, const float* __restrict__ phi_v, int nsched, const int* __restrict__ step,
    double* __restrict__ ws) {
    const int clip = blockIdx.y;
    const RescaleClip rc = rescale_clip(clip, scale, phi, scale_v, phi_v, nsched, step);
    if (!rc.active) return;
    const int64_t n = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t pair = (int64_t)rows * C * Ft * HW;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < RESCALE_PER_THREAD; ++k) {
        const int64_t e = (int64_t)blockIdx.x * SEER_RESCALE_TILE + k * RESCALE_THREADS + threadIdx.x;
        if (e >= n) break;
        const double c = (double)eps[rescale_offset(clip, C, Ft, cond_f, HW, e) + pair];
        const double g = (double)cfg_eps_at(eps, 1, rows, C, Ft, cond_f, HW, rc.scale, (int64_t)clip * n + e);
        s[0] += c, s[1] += c * c, s[2] += g, s[3] += g * g;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int j = 0; j < 4; ++j) s[j] += __shfl_xor(s[j], off);
    __shared__ double part[RESCALE_THREADS / 64][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < 4; ++j) part[wave][j] = s[j];
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = part[0][threadIdx.x];
        for (int w = 1; w < RESCALE_THREADS / 64; ++w) t += part[w][threadIdx.x];
        ws[((int64_t)clip * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = t;
    }
}

// the multiplier of a clip from its four sums; q_g <= 0 (a constant clip, n = 1) or a ratio that is not finite: 1, where diffusers
// divides by a zero std
__device__ __forceinline__ float rescale_multiplier(const double* s, int64_t n, float phi) {
    const double nn = (double)n;
    const double qc = fmax(nn * s[1] - s[0] * s[0], 0.0);
    const double qg = nn * s[3] - s[2] * s[2];
    if (!(qg > 0.0)) return 1.f;
    const double r = qc / qg;
    if (!isfinite(r)) return 1.f;
    return (float)((double)phi * sqrt(r) + (1.0 - (double)phi));
}

__global__ __launch_bounds__(RESCALE_THREADS) void cfg_rescale_apply_kernel(
    float* eps, int rows, int C, int Ft, int cond_f, int HW, float scale, float phi, const float* __restrict__ scale_v,
    const float* __restrict__ phi_v, int nsched, const int* __restrict__ step, const double* __restrict__ ws,
    float* __restrict__ mult) {
    const int clip = blockIdx.y;
    const RescaleClip rc = rescale_clip(clip, scale, phi, scale_v, phi_v, nsched, step);
    if (!rc.active) return;
    const int64_t n = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t pair = (int64_t)rows * C * Ft * HW;
    __shared__ float m_shared;
    if (threadIdx.x == 0) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const double* w = ws + (int64_t)clip * gridDim.x * 4;
        for (unsigned p = 0; p < gridDim.x; ++p)
            for (int j = 0; j < 4; ++j) s[j] += w[4 * (int64_t)p + j];
        const float m = rescale_multiplier(s, n, rc.phi);
        m_shared = m;
        if (blockIdx.x == 0 && mult) mult[clip] = m;
    }
    __syncthreads();
    const float m = m_shared;
    for (int k = 0; k < RESCALE_PER_THREAD; ++k) {
        const int64_t e = (int64_t)blockIdx.x * SEER_RESCALE_TILE + k * RESCALE_THREADS + threadIdx.x;
        if (e >= n) break;
        const int64_t off = rescale_offset(clip, C, Ft, cond_f, HW, e);
        const float v = m * cfg_eps_at(eps, 1, rows, C, Ft, cond_f, HW, rc.scale, (int64_t)clip * n + e);
        eps[off] = v;
        eps[off + pair] = v;
    }
}

// ---- GIVEN latents (masked sampling, stochastic_encode; CompVis ldm/models/diffusion/ddim.py:144-147, 207-221): q(e) is the given
// latent x0 noised to the level of coefficient row `index`, its noise n either read from a tensor or normal e of Philox stream 2 of
// the clip's seed at that index.  One expression for the three kernels below, so the seeded form gets the bits of the noise-tensor
// form fed seer_philox_normal(seed, 2, index).
__device__ __forceinline__ float q_known(const float* __restrict__ coef, int index, float x0v, float n) {
    return sqrtf(coef[4 * index]) * x0v + coef[4 * index + 3] * n;
}

__device__ __forceinline__ float known_noise(const float* __restrict__ noise, int64_t i, const uint32_t* __restrict__ seed, int index,
                                             uint32_t el) {
    return noise ? noise[i] : seer_philox::normal_at(seed[0], seed[1], seer_philox::STREAM_KNOWN, (uint32_t)index, el);
}

// the blend of one element: m == 0 leaves the word alone (nothing is read but the mask, nothing drawn), m == 1 selects q whatever
// x holds, anything else is CompVis's img_orig * mask + (1. - mask) * img
__device__ __forceinline__ void known_blend_at(float* x, float m, const float* __restrict__ known, const float* __restrict__ coef,
                                               int index, const float* __restrict__ noise, const uint32_t* __restrict__ seed,
                                               uint32_t el, int64_t i) {
    if (m == 0.f) return;
    const float q = q_known(coef, index, known[i], known_noise(noise, i, seed, index, el));
    x[i] = m == 1.f ? q : q * m + (1.f - m) * x[i];
}

// out[bi][e] = q with row index[bi] of coef; a row whose index is outside 0 .. nsched - 1 is not written
__global__ void q_sample_kernel(const float* __restrict__ x0, int b, int64_t per_row, const float* __restrict__ coef, int nsched,
                                const int* __restrict__ index, const float* __restrict__ noise, const uint32_t* __restrict__ seeds,
                                float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)b * per_row) return;
    const int64_t bi = i / per_row;
    const int idx = index[bi];
    if (idx < 0 || idx >= nsched) return;
    out[i] = q_known(coef, idx, x0[i], known_noise(noise, i, seeds + 2 * bi, idx, (uint32_t)(i - bi * per_row)));
}

// x [b, C, Fp, HW] in place; mask [b, Fp, HW] is broadcast over channels.  step != nullptr: index = step[0], the NEXT step's index
// (this kernel runs in front of seer_ddim_step_begin); it is only read.
__global__ void known_blend_kernel(float* x, const float* __restrict__ mask, const float* __restrict__ known, int b, int C, int Fp,
                                   int HW, const float* __restrict__ coef, int index, const int* __restrict__ step,
                                   const float* __restrict__ noise, const uint32_t* __restrict__ seeds) {
    const int64_t per_frames = (int64_t)Fp * HW, per_clip = per_frames * C;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) index = step[0];
    if (index < 0 || i >= (int64_t)b * per_clip) return;
    const int64_t bi = i / per_clip;
    const int64_t el = i - bi * per_clip;
    known_blend_at(x, mask[bi * per_frames + el % per_frames], known, coef, index, noise, seeds + 2 * bi, (uint32_t)el, i);
}

// the same over slots, seeded: index = step[s][0] and coef[s]; an idle slot (index < 0 or >= nsched) writes nothing
__global__ void slot_known_blend_kernel(float* x, const float* __restrict__ mask, const float* __restrict__ known, int slots, int C,
                                        int Fp, int HW, const float* __restrict__ coef, int nsched, const int* __restrict__ step,
                                        const uint32_t* __restrict__ seeds) {
    const int64_t per_frames = (int64_t)Fp * HW, per_slot = per_frames * C;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int64_t s = i / per_slot;
    const int index = step[2 * s];
    if (index < 0 || index >= nsched) return;
    const int64_t el = i - s * per_slot;
    known_blend_at(x, mask[s * per_frames + el % per_frames], known, coef + s * nsched * 4, index, nullptr, seeds + 2 * s, (uint32_t)el,
                   i);
}

// ---- host side: every export states its own NULL and range conditions, then launches through launch_per_element.  One export per
// kernel: the mode is read from which pointers are set, each mode keeps its own checks, and a half-set mode is refused ---------------
// exactly one index source: the host's `index` with no step words, or the step words with index == SEER_INDEX_FROM_STEP
inline bool index_source_ok(int32_t index, const void* step) { return step ? index == SEER_INDEX_FROM_STEP : index >= 0; }

// the latent a step updates, [rows, C, F_total - cond_f, HW]
inline bool update_shape_ok(int32_t C, int32_t F_total, int32_t cond_f, int32_t HW) {
    return C > 0 && HW > 0 && cond_f >= 0 && cond_f < F_total;
}

// the seeded forms: a clip's element index is a 32-bit Philox counter word times four, so a clip stays below 2^31 elements
inline bool philox_clip_ok(int32_t C, int32_t F_total, int32_t cond_f, int32_t HW) {
    return update_shape_ok(C, F_total, cond_f, HW) && (int64_t)C * ((int64_t)F_total - cond_f) * HW < ((int64_t)1 << 31);
}

// the UNet input a begin kernel assembles, [reps * rows, C, f1 + F_pred, HW]
inline bool begin_shape_ok(const float* x0_emb, int32_t C, int32_t f1, int32_t F_pred, int32_t HW) {
    return C > 0 && f1 >= 0 && F_pred > 0 && HW > 0 && (f1 == 0 || x0_emb);
}

inline int64_t elements(int32_t rows, int32_t C, int64_t F, int32_t HW) { return (int64_t)rows * C * F * HW; }

// one thread per element, 256 to a block.  `aligned`: the pointers (NULL passes) the export refuses unless they are 4-byte aligned --
// the slot, seeded and given-latents kernels rely on that and no more, the int64 tables included.  A grid beyond one dimension is
// refused.
using Pointers = std::initializer_list<const void*>;

template <typename... P, typename... A>
int launch_per_element(void (*kernel)(P...), int64_t n, Pointers aligned, void* stream, A... args) {
    for (const void* p : aligned)
        if (reinterpret_cast<uintptr_t>(p) & 3) return SEER_EINVAL;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), args...);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

}  // namespace

// at most one of noise and seeds; the seeded mode alone bounds the clip and asks for aligned pointers, and it alone reads temperature
extern "C" int seer_cfg_ddim_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                  int32_t HW, float scale, const float* coef, int32_t index, int32_t* step, const float* x,
                                  const float* noise, const uint32_t* seeds, float temperature, float* x_prev, float* pred_x0,
                                  void* stream) {
    if (!eps || !coef || !x || !x_prev || b <= 0 || !index_source_ok(index, step) || (noise && seeds) ||
        !(seeds ? philox_clip_ok(C, F_total, cond_f, HW) : update_shape_ok(C, F_total, cond_f, HW)))
        return SEER_EINVAL;
    return launch_per_element(cfg_ddim_kernel, elements(b, C, F_total - cond_f, HW),
                              seeds ? Pointers{eps, coef, step, x, seeds, x_prev, pred_x0} : Pointers{}, stream, eps, cfg, b, C, F_total,
                              cond_f, HW, scale, coef, step ? 0 : index, step, x, noise, seeds, seeds ? temperature : 0.f, x_prev, pred_x0);
}

extern "C" int seer_ddim_step_begin(const float* x0_emb, const float* x, int32_t b, int32_t reps, int32_t C, int32_t f1,
                                    int32_t F_pred, int32_t HW, const int64_t* t_table, int32_t* step, float* sample,
                                    int64_t* t_out, void* stream) {
    if (!x || !t_table || !step || !sample || !t_out || b <= 0 || reps <= 0 || !begin_shape_ok(x0_emb, C, f1, F_pred, HW))
        return SEER_EINVAL;
    return launch_per_element(ddim_assemble_kernel, elements(b, C, f1 + F_pred, HW), {}, stream, x0_emb, x, b, reps, C, f1, F_pred, HW,
                              t_table, step, sample, t_out);
}

// the device form carries its limit word, the host form has none
extern "C" int seer_cfg_ddim_invert_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                         int32_t HW, float scale, const float* coef, int32_t index, int32_t* step,
                                         const int32_t* limit, const float* x, float* x_next, float* pred_x0, void* stream) {
    if (!eps || !coef || !x || !x_next || b <= 0 || !update_shape_ok(C, F_total, cond_f, HW) || !index_source_ok(index, step) ||
        (limit != nullptr) != (step != nullptr))
        return SEER_EINVAL;
    return launch_per_element(cfg_ddim_invert_kernel, elements(b, C, F_total - cond_f, HW), {eps, coef, step, limit, x, x_next, pred_x0},
                              stream, eps, cfg, b, C, F_total, cond_f, HW, scale, coef, step ? 0 : index, step, limit, x, x_next, pred_x0);
}

extern "C" int seer_cfg_plms_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                  int32_t HW, float scale, const float* coef, int32_t index, int32_t order, const float* x,
                                  const float* h1, const float* h2, const float* h3, float* x_prev, float* pred_x0, float* e_out,
                                  void* stream) {
    if (!eps || !coef || !x || !x_prev || b <= 0 || !update_shape_ok(C, F_total, cond_f, HW) || index < 0 || order < 0 || order > 4 ||
        (order >= 1 && !h1) || (order >= 3 && !h2) || (order >= 4 && !h3))
        return SEER_EINVAL;
    return launch_per_element(cfg_plms_kernel, elements(b, C, F_total - cond_f, HW), {}, stream, eps, cfg, b, C, F_total, cond_f, HW,
                              scale, coef, index, order, x, h1, h2, h3, x_prev, pred_x0, e_out);
}

extern "C" int seer_cfg_plms_step_dev(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                      int32_t HW, float scale, const float* coef, int32_t* step, float* ring, int32_t* ring_state,
                                      const float* x, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !coef || !step || !ring || !ring_state || !x || !x_prev || b <= 0 || !update_shape_ok(C, F_total, cond_f, HW))
        return SEER_EINVAL;
    return launch_per_element(cfg_plms_dev_kernel, elements(b, C, F_total - cond_f, HW), {}, stream, eps, cfg, b, C, F_total, cond_f, HW,
                              scale, coef, step, ring, ring_state, x, x_prev, pred_x0);
}

// host form: `order` 1 or 2, d_prev at order 2.  Device form: step and state, and pred_x0 is the history -- the kernel reads it as
// d_prev and takes its order from state
extern "C" int seer_cfg_dpm_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                 float scale, const float* x, const float* coef, int32_t nsched, int32_t index, int32_t order,
                                 int32_t* step, int32_t* state, const float* d_prev, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !x || !coef || !x_prev || b <= 0 || !update_shape_ok(C, F_total, cond_f, HW) || nsched < 1 ||
        !index_source_ok(index, step) || (state != nullptr) != (step != nullptr) ||
        (step ? !pred_x0 || d_prev : index >= nsched || (order != 1 && order != 2) || (order == 2 && !d_prev)))
        return SEER_EINVAL;
    return launch_per_element(cfg_dpm_kernel, elements(b, C, F_total - cond_f, HW), {eps, x, coef, step, state, d_prev, x_prev, pred_x0},
                              stream, eps, cfg, b, C, F_total, cond_f, HW, scale, coef, nsched, step ? 0 : index, step ? 1 : order, step,
                              state, x, step ? pred_x0 : d_prev, x_prev, pred_x0);
}

// x_prov and state go together (NULL both: every slot is read as phase 0)
extern "C" int seer_slot_step_begin(const float* x0_emb, const float* x, const float* x_prov, int32_t slots, int32_t reps, int32_t C,
                                    int32_t f1, int32_t F_pred, int32_t HW, const int64_t* t_table, int32_t nsched, int32_t* step,
                                    int32_t* state, float* sample, int64_t* t_out, void* stream) {
    if (!x || !t_table || !step || !sample || !t_out || (x_prov != nullptr) != (state != nullptr) || slots < 1 || nsched < 1 ||
        (reps != 1 && reps != 2) || !begin_shape_ok(x0_emb, C, f1, F_pred, HW) || x_prov == x)
        return SEER_EINVAL;
    return launch_per_element(slot_assemble_kernel, elements(slots, C, (int64_t)f1 + F_pred, HW),
                              {x0_emb, x, x_prov, t_table, step, state, sample, t_out}, stream, x0_emb, x, x_prov, slots, reps, C, f1,
                              F_pred, HW, reinterpret_cast<const int*>(t_table), nsched, step, state, sample,
                              reinterpret_cast<int*>(t_out));
}

// seeds and temperature go together (NULL both: eta = 0); the seeded mode alone bounds the clip
extern "C" int seer_slot_cfg_ddim_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                       const float* scale, const float* coef, int32_t nsched, int32_t* step, const float* x,
                                       const uint32_t* seeds, const float* temperature, float* x_prev, float* pred_x0,
                                       void* stream) {
    if (!eps || !scale || !coef || !step || !x || !x_prev || (seeds != nullptr) != (temperature != nullptr) || slots < 1 ||
        nsched < 1 || !(seeds ? philox_clip_ok(C, F_total, cond_f, HW) : update_shape_ok(C, F_total, cond_f, HW)))
        return SEER_EINVAL;
    return launch_per_element(slot_cfg_ddim_kernel, elements(slots, C, (int64_t)F_total - cond_f, HW),
                              {eps, scale, coef, step, x, seeds, temperature, x_prev, pred_x0}, stream, eps, slots, C, F_total, cond_f,
                              HW, scale, coef, nsched, step, x, seeds, temperature, x_prev, pred_x0);
}

extern "C" int seer_slot_cfg_plms_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                       const float* scale, const float* coef, int32_t nsched, int32_t* step, int32_t* state,
                                       float* ring, const float* x, float* x_prov, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !scale || !coef || !step || !state || !ring || !x || !x_prov || !x_prev || slots < 1 || nsched < 1 ||
        !update_shape_ok(C, F_total, cond_f, HW) || x_prov == x)
        return SEER_EINVAL;
    return launch_per_element(slot_cfg_plms_kernel, elements(slots, C, (int64_t)F_total - cond_f, HW),
                              {eps, scale, coef, step, state, ring, x, x_prov, x_prev, pred_x0}, stream, eps, slots, C, F_total, cond_f,
                              HW, scale, coef, nsched, step, state, ring, x, x_prov, x_prev, pred_x0);
}

// slots 1..4 (the [uc | c] rows of all slots go through the 8-row time embedding); d_hist is read and written, so it is neither x
// nor x_prev
extern "C" int seer_slot_cfg_dpm_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                      const float* scale, const float* coef, const float* dpm_coef, int32_t nsched, int32_t* step,
                                      int32_t* state, const float* x, float* x_prev, float* d_hist, void* stream) {
    if (!eps || !scale || !coef || !dpm_coef || !step || !state || !x || !x_prev || !d_hist || slots < 1 || slots > 4 || nsched < 1 ||
        !update_shape_ok(C, F_total, cond_f, HW) || d_hist == x || d_hist == x_prev)
        return SEER_EINVAL;
    return launch_per_element(slot_cfg_dpm_kernel, elements(slots, C, (int64_t)F_total - cond_f, HW),
                              {eps, scale, coef, dpm_coef, step, state, x, x_prev, d_hist}, stream, eps, slots, C, F_total, cond_f, HW,
                              scale, coef, dpm_coef, nsched, step, state, x, x_prev, d_hist);
}

// v-prediction: the model output converted to eps in front of an update kernel; reps 1 (no CFG) or 2 (the [uc | c] pair); out may be v
extern "C" int seer_v_to_eps(const float* v, int32_t reps, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                             const float* coef, int32_t nsched, int32_t index, const int32_t* step, const float* x, float* out,
                             void* stream) {
    if (!v || !coef || !x || !out || (reps != 1 && reps != 2) || b <= 0 || !update_shape_ok(C, F_total, cond_f, HW) || nsched < 1 ||
        !index_source_ok(index, step) || index >= nsched)
        return SEER_EINVAL;
    return launch_per_element(v_to_eps_kernel, reps * elements(b, C, (int64_t)F_total - cond_f, HW), {v, coef, step, x, out}, stream, v,
                              reps, b, C, F_total, cond_f, HW, coef, nsched, step ? 0 : index, step, x, out);
}

// state and x_prov go together (NULL both: every slot is read as phase 0); slots 1..4 as in the slot updates' widest form
extern "C" int seer_slot_v_to_eps(const float* v, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                  const float* coef, int32_t nsched, const int32_t* step, const int32_t* state, const float* x,
                                  const float* x_prov, float* out, void* stream) {
    if (!v || !coef || !step || !x || !out || (state != nullptr) != (x_prov != nullptr) || slots < 1 || slots > 4 || nsched < 1 ||
        !update_shape_ok(C, F_total, cond_f, HW) || x_prov == x)
        return SEER_EINVAL;
    return launch_per_element(slot_v_to_eps_kernel, 2 * elements(slots, C, (int64_t)F_total - cond_f, HW),
                              {v, coef, step, state, x, x_prov, out}, stream, v, slots, C, F_total, cond_f, HW, coef, nsched, step, state,
                              x, x_prov, out);
}

// guidance rescale: two launches over (tiles of a clip, clips); the solo and the slot export differ in where scale and phi come from
namespace {

inline int64_t rescale_tiles(int32_t C, int32_t F_total, int32_t cond_f, int32_t HW) {
    return (elements(1, C, (int64_t)F_total - cond_f, HW) + SEER_RESCALE_TILE - 1) / SEER_RESCALE_TILE;
}

int launch_rescale(float* out, int32_t clips, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, float scale, float phi,
                   const float* scale_v, const float* phi_v, int32_t nsched, const int32_t* step, double* ws, float* mult,
                   void* stream) {
    for (const void* p : Pointers{out, scale_v, phi_v, step, mult})
        if (reinterpret_cast<uintptr_t>(p) & 3) return SEER_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) & 7) return SEER_EINVAL;
    const int64_t tiles = rescale_tiles(C, F_total, cond_f, HW);
    if (tiles > 0x7fffffff || clips > 65535) return SEER_EINVAL;
    const dim3 grid((unsigned)tiles, (unsigned)clips), block(RESCALE_THREADS);
    hipLaunchKernelGGL(cfg_rescale_moments_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), out, clips, C, F_total,
                       cond_f, HW, scale, phi, scale_v, phi_v, nsched, step, ws);
    SEER_LAUNCH_CHECK();
    hipLaunchKernelGGL(cfg_rescale_apply_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), out, clips, C, F_total,
                       cond_f, HW, scale, phi, scale_v, phi_v, nsched, step, ws, mult);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

}  // namespace

extern "C" int64_t seer_cfg_rescale_ws_bytes(int32_t clips, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW) {
    if (clips <= 0 || !update_shape_ok(C, F_total, cond_f, HW)) return SEER_EINVAL;
    return (int64_t)clips * rescale_tiles(C, F_total, cond_f, HW) * 4 * (int64_t)sizeof(double);
}

extern "C" int seer_cfg_rescale(float* out, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, float scale,
                                float rescale, double* ws, float* mult, void* stream) {
    if (!out || !ws || b <= 0 || !update_shape_ok(C, F_total, cond_f, HW) || !(rescale >= 0.f && rescale <= 1.f))
        return SEER_EINVAL;
    if (rescale == 0.f) return SEER_OK;
    return launch_rescale(out, b, C, F_total, cond_f, HW, scale, rescale, nullptr, nullptr, 1, nullptr, ws, mult, stream);
}

// slots 1..4 as in the other slot forms; phi is the host's to validate (submit), nothing is clamped here
extern "C" int seer_slot_cfg_rescale(float* out, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                     const float* scale, const float* rescale, int32_t nsched, const int32_t* step, double* ws,
                                     float* mult, void* stream) {
    if (!out || !scale || !rescale || !step || !ws || slots < 1 || slots > 4 || nsched < 1 || !update_shape_ok(C, F_total, cond_f, HW))
        return SEER_EINVAL;
    return launch_rescale(out, slots, C, F_total, cond_f, HW, 0.f, 0.f, scale, rescale, nsched, step, ws, mult, stream);
}

// given latents: exactly one of noise and seeds; a clip's element index is a Philox counter word, as in the seeded steps
extern "C" int seer_q_sample(const float* x0, int32_t b, int64_t per_row, const float* coef, int32_t nsched, const int32_t* index,
                             const float* noise, const uint32_t* seeds, float* out, void* stream) {
    if (!x0 || !coef || !index || !out || (noise != nullptr) == (seeds != nullptr) || b <= 0 || nsched < 1 || per_row <= 0 ||
        per_row >= ((int64_t)1 << 31))
        return SEER_EINVAL;
    return launch_per_element(q_sample_kernel, (int64_t)b * per_row, {x0, coef, index, noise, seeds, out}, stream, x0, b, per_row, coef,
                              nsched, index, noise, seeds, out);
}

extern "C" int seer_known_blend(float* x, const float* mask, const float* known, int32_t b, int32_t C, int32_t F_pred, int32_t HW,
                                const float* coef, int32_t index, const int32_t* step, const float* noise, const uint32_t* seeds,
                                void* stream) {
    if (!x || !mask || !known || !coef || (noise != nullptr) == (seeds != nullptr) || b <= 0 || !philox_clip_ok(C, F_pred, 0, HW))
        return SEER_EINVAL;
    return launch_per_element(known_blend_kernel, elements(b, C, F_pred, HW), {x, mask, known, coef, step, noise, seeds}, stream, x, mask,
                              known, b, C, F_pred, HW, coef, index, step, noise, seeds);
}

extern "C" int seer_slot_known_blend(float* x, const float* mask, const float* known, int32_t slots, int32_t C, int32_t F_pred,
                                     int32_t HW, const float* coef, int32_t nsched, const int32_t* step, const uint32_t* seeds,
                                     void* stream) {
    if (!x || !mask || !known || !coef || !step || !seeds || slots < 1 || nsched < 1 || !philox_clip_ok(C, F_pred, 0, HW))
        return SEER_EINVAL;
    return launch_per_element(slot_known_blend_kernel, elements(slots, C, F_pred, HW), {x, mask, known, coef, step, seeds}, stream, x,
                              mask, known, slots, C, F_pred, HW, coef, nsched, step, seeds);
}
