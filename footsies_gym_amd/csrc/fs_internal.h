// Internal interface between the host C-ABI (fs_api.cpp) and the HIP kernels
// (fs_kernels.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/footsies.h"

namespace fsk {

// BattleAI's input plans (AI:192-312): the queue of a plan holds plan_len inputs, so a queue
// index is always below its plan's length (host validation and the kernels' code tables).
enum { MP_NEUTRAL, MP_FAR1, MP_FAR2, MP_MID1, MP_MID2, MP_FALLBACK1, MP_FALLBACK2 };
enum { AP_NONE, AP_ONE_HIT, AP_TWO_HIT, AP_IMMEDIATE_SPECIAL, AP_DELAY_SPECIAL };
constexpr uint32_t move_plan_len(uint32_t plan) {  // AI:192-253
  return plan == MP_FAR1 ? 90u : plan == MP_FAR2 ? 56u : plan == MP_MID1 ? 70u : plan == MP_MID2 ? 33u
       : plan == MP_FALLBACK1 ? 60u : plan == MP_FALLBACK2 ? 63u : 30u;
}
constexpr uint32_t attack_plan_len(uint32_t plan) {  // AI:255-312
  return plan == AP_ONE_HIT ? 19u : plan == AP_TWO_HIT ? 23u : plan == AP_IMMEDIATE_SPECIAL ? 61u
       : plan == AP_DELAY_SPECIAL ? 121u : 30u;
}

// Per-arena state in HBM, struct-of-arrays (one element per arena, 8/16-byte
// vectors so one wave64 load/store moves 512 B / 1 KiB contiguous).
struct DevState {
  float2* pos;     // x of P1, P2 (Fighter.position.x)
  uint2* hist;     // per fighter: bit j = backward on input[j], bit 16 + j = forward (facing-relative)
  uint4* fpk;      // packed fighter words: (P1 lo, P1 hi, P2 lo, P2 hi), layout in fs_kernels.hip
  int2* aw;        // (frameCount, arena header word)
  double* cum;     // FootsiesEnv._cummulative_episode_reward
  uint4* rng;      // the game's UnityEngine.Random Xorshift128 state (every mode)
  uint2* bot;      // P2's BattleAI: (bot word, previous FightState distance bits), layout in fs_kernels.hip
  uint2* bot1;     // P1's BattleAI (FS_P1_BOT), same layout
  float2* posy;    // y of P1, P2 (Fighter.position.y): 0 unless a state load set it (general geometry)
};

// The kernels' P2 variants.  FS_P2_EXTERNAL / FS_P2_BOT / FS_P2_NOOP run handles whose actors are
// fixed and uniform (P1 the agent; P2 remote, the bot, or idle); kActors runs per-arena actors: a
// P1 bot (FS_P1_BOT) and / or P2 switched between remote and bot (fs_set_p2_mode).
constexpr int kActors = 3;

struct DevOutputs {
  uint8_t* guard;
  uint8_t* move;
  float* move_frame;
  float* position;
  double* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  int32_t* frame;
  uint8_t* action;
  uint8_t* hitstun;
  uint8_t* final_guard;
  uint8_t* final_move;
  float* final_move_frame;
  float* final_position;
  int32_t* final_frame;
  uint8_t* final_action;
  uint8_t* final_hitstun;
  // fs_step_n_packed (include/footsies.h fs_packed_traj): lane records of 16 B, with `reward`
  // above as the trajectory's reward; the per-field pointers are then unused
  uint4* pk_lanes;
  uint4* pk_final;
};

// the in-kernel actor of fs_step_n_policy (fs_policy.h): fp32 weights in torch layouts
struct PolicyParams {
  const float *w1, *b1, *w2, *b2, *w3, *b3;  // [64][8] [64] [64][64] [64] [8][64] [8]
  uint8_t* actions;  // [n][N] or null
  float* logp;       // [n][N] or null
  uint64_t seed;
};

struct StepParams {
  DevState st;
  DevOutputs out;
  PolicyParams pol;
  const uint8_t* p1;   // [n][N] or null (hashed)
  const uint8_t* p2;   // [n][N] or null
  const uint8_t* active;  // [N] or null: single-tick launches skip arenas whose byte is 0
  uint64_t action_seed;
  uint64_t t0;         // global step index of the first tick (hash counter)
  uint64_t arena_base; // global index of arena 0 (fs_config.arena_base): hash / sampling keys
  int n_envs;
  int n_steps;
  int out_stride_steps;  // 1: outputs are [n][N] trajectories; 0: overwrite one [N] set
  int dense_reward;
  int autoreset_mode;
  int p1_bot;     // kActors: P1 is the bot (FS_P1_BOT)
  int p2_resets;  // kActors: P2's bot is Reset at Intro (the handle was created with FS_P2_BOT)
  int p2_noop;    // kActors: a non-bot P2 presses nothing (FS_P2_NOOP handle)
  int prio;       // fused launches: time-sliced wave priority (set by the launcher, prio_slice)
  int geom;       // some arena has position.y != 0 or a flipped facing: the general-geometry tick
  int prefetch;   // two-lane fused row launches: each tick's request prepared at the end of the tick before
  uint2* rec;     // one-tick launches (fs_step_rec): each arena's FS_RECORD_BYTES record, or null
  // host actions of a one-tick launch over at most kInlineArenas arenas, carried in the kernel
  // arguments instead of a staging copy (inl_n != 0): byte a of inl[player] is arena a's input
  int inl_n;
  uint32_t inl[2][8];
};
constexpr int kInlineArenas = 32;  // sizeof(StepParams::inl[0])

// fs_step_skip (k_step_skip): one launch runs each active arena to its next agent decision
struct SkipParams {
  StepParams p;          // p.p1: [N] or null (resume); p.active: [N] or null
  double* acc;           // [N] the handle's reward sums of the current decision
  int32_t* nticks;       // [N] the handle's tick counts of the current decision
  int32_t* ticks_out;    // [N] or null
  uint8_t* pending_out;  // [N] or null; may alias p.active (read before the loop, written after it)
  int32_t* n_pending;    // [1] or null: zeroed by the host on the stream ahead of the launch
  int max_ticks;         // >= 1
  int resume;            // continue the decision with input 0 from acc / nticks
};

// fs_step_skip_policy (k_step_skip_policy): one launch runs p.n_steps agent decisions per arena, the
// actor p.pol inside; every output row is a decision's (p.pol.actions / logp, ticks_out, capped_out: [n][N])
struct SkipPolicyParams {
  StepParams p;         // p.n_steps: decisions; p.t0: the first decision's index (the sampling counter)
  int32_t* ticks_out;   // [n][N] or null
  uint8_t* capped_out;  // [n][N] or null
  int max_ticks;        // >= 1: closes a decision
};

// fs_step_n_selfplay (k_step_n_selfplay): k_step_n_policy's launch with a second actor for P2
struct SelfPlayParams {
  StepParams p;       // p.pol: P1's actor; p.p1 / p.p2 unused (no action rows)
  PolicyParams pol2;  // P2's actor: its own weights, seed and [n][N] outputs
  int mirror;         // FS_SELFPLAY_MIRROR: P2 sees the game from its own side, Left / Right exchanged
};

// fs_step_skip_selfplay (k_step_skip_selfplay): p.n_steps agent decisions per arena, P2's actor on every tick
struct SkipSelfPlayParams {
  StepParams p;         // p.pol: P1's actor, its outputs [n][N] by decision; p.t0: the first decision's index
  PolicyParams pol2;    // P2's actor; its outputs [n][max_ticks][N] by (decision, tick) or null
  int32_t* ticks_out;   // [n][N] or null
  uint8_t* capped_out;  // [n][N] or null
  int max_ticks;        // >= 1: closes a decision
  int mirror;           // FS_SELFPLAY_MIRROR
};

// fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool: P2's weights of the two launches above chosen per
// block (kBlock / 2 = FS_SELFPLAY_GROUP arenas) from a pool of actors; pol2's six weight pointers are unused
struct PoolParams {
  const float* weights;  // [n_slots][FS_PPO_ACTOR_PARAMS], a slot = w1 | b1 | w2 | b2 | w3 | b3
  const uint8_t* slot;   // [blocks of the launch]: block b stages slot min(slot[b], n_slots - 1)
  int n_slots;           // >= 1
};
struct SelfPlayPoolParams {
  SelfPlayParams q;
  PoolParams pool;
};
struct SkipSelfPlayPoolParams {
  SkipSelfPlayParams q;
  PoolParams pool;
};

struct ResetParams {
  DevState st;
  DevOutputs out;
  const uint64_t* seeds;  // [N] or null
  const uint8_t* mask;    // [N] or null
  int n_envs;
  int flags;
  int init;  // 1: fresh arenas (`new Fighter()`), seeds from base_seed
  uint64_t base_seed;
  uint64_t arena_base;
  int p1_bot, p2_mode;  // the handle's actors (fs_config p1_mode / p2_mode)
};

// FootsiesEnv's delayed-frame queue (FE:126-131, 493-504, 532-535) for frame_delay = d > 0:
// per arena a ring of d packed observation records and a head slot that advances with the
// arena's own steps.  Applied after a step kernel to the rows it wrote, or after a reset to
// refill the rings of the arenas it reset (output frame == -1).
struct DelayParams {
  DevOutputs out;
  uint4* ring;          // [d][N] records of 2 x uint4 (layout in fs_delay.hip)
  int n_envs;
  int delay;            // d
  int n_steps;          // rows to process (1 for fs_step / fs_reset)
  int out_stride_steps;
  uint16_t* head;       // [N] per arena: the ring slot its next step reads and overwrites (< d)
  const uint8_t* active;  // fs_step_masked / a masked fs_reset: only these arenas stepped / were reset (nullptr = all)
  int refill_only;      // 1: after fs_reset / fs_create (no queue shift)
  int same_step;        // FS_AUTORESET_SAME_STEP: a terminal row's final_* take the delayed record
};

// launchers (fs_kernels.hip, fs_delay.hip); return hipError_t of the launch
// variant: FS_P2_EXTERNAL / FS_P2_BOT / FS_P2_NOOP or kActors (see above)
hipError_t launch_step(const StepParams& p, int float_mode, int variant, hipStream_t s);
const char* step_kernel_name(bool policy, bool hashed, int n_steps, int n_envs, int float_mode, int variant,
                             bool geom, bool packed, int autoreset_mode);
// p2_mode: FS_P2_BOT or FS_P2_NOOP (the handle's fixed P2; fs_step_skip refuses the others)
hipError_t launch_step_skip(const SkipParams& q, int float_mode, int p2_mode, hipStream_t s);
hipError_t launch_step_skip_policy(const SkipPolicyParams& q, int float_mode, int p2_mode, hipStream_t s);
const char* step_skip_policy_kernel_name(int float_mode, int p2_mode);
// (FS_P2_EXTERNAL handles with no arena switched to the bot; fs_step_n_selfplay refuses the others)
// pool: null for one opponent (q.pol2's weights), else the pool kernel with P2's weights per block
hipError_t launch_step_selfplay(const SelfPlayParams& q, const PoolParams* pool, int float_mode, hipStream_t s);
const char* step_selfplay_kernel_name(int float_mode, bool pool);
hipError_t launch_step_skip_selfplay(const SkipSelfPlayParams& q, const PoolParams* pool, int float_mode, hipStream_t s);
const char* step_skip_selfplay_kernel_name(int float_mode, bool pool);
// fs_step_n_league / fs_step_skip_league: the pool launches on a handle whose groups of FS_SELFPLAY_GROUP arenas
// are each all remote or all switched to the bot (the caller checks); a bot group's block runs P1's actor
// against the arena's BattleAI and ignores the pool
hipError_t launch_step_league(const SelfPlayParams& q, const PoolParams& pool, int float_mode, hipStream_t s);
hipError_t launch_step_skip_league(const SkipSelfPlayParams& q, const PoolParams& pool, int float_mode, hipStream_t s);
const char* step_league_kernel_name(int float_mode, bool skip);
hipError_t launch_reset(const ResetParams& p, int float_mode, hipStream_t s);
hipError_t launch_set_p2(const DevState& st, int bot, const uint8_t* mask, int n, hipStream_t s);
hipError_t launch_hash_actions(int n_envs, int n_steps, uint64_t seed, uint64_t t0, uint64_t arena_base, uint8_t* p1,
                               uint8_t* p2, hipStream_t s);
hipError_t launch_get_state(const DevState& st, fs_arena_state* dst, fs_env_state* env_dst, int n, hipStream_t s);
hipError_t launch_set_state(const DevState& st, const fs_arena_state* src, int n, hipStream_t s);
hipError_t launch_delay(const DelayParams& p, hipStream_t s);
hipError_t launch_pack_records(const DevOutputs& o, void* dst, int n, hipStream_t s);
// fs_learn.hip: the C5 learner's minibatch gradient (fs_ppo_grad)
size_t ppo_workspace_bytes();
hipError_t launch_ppo_grad(const float* rows, int64_t n, const float* const actor[6], const float* const critic[6],
                           float clip, float vf_coef, float ent_coef, float* grad, float* loss, void* workspace,
                           hipStream_t s, bool split, const int64_t* runs = nullptr, int run_shift = 0,
                           int64_t n_rows = 0);
hipError_t launch_ppo_eval(const float* x, int64_t n_values, const uint8_t* actions, int64_t n_logp,
                           const float* const actor[6], const float* const critic[6], float* values, float* logp,
                           void* workspace, hipStream_t s, bool split);
hipError_t launch_ppo_gae(const double* rew, const uint8_t* done, const float* val, int T, int64_t N, float gamma,
                          float gamma_lam, float* adv, float* ret, hipStream_t s);
hipError_t launch_ppo_features(const uint8_t* guard, const uint8_t* move, const float* move_frame,
                               const float* position, int64_t n, float* out, hipStream_t s);
hipError_t launch_ppo_pack(const float* x, const uint8_t* act, const float* old, const float* adv, const float* ret,
                           const float* stats, int64_t n, float* rows, hipStream_t s);
// P2's side of a self-play trajectory over a selection of the arenas (fs_ppo_features_p2 / fs_ppo_gae_p2)
hipError_t launch_ppo_features_p2(const uint8_t* guard, const uint8_t* move, const float* move_frame,
                                  const float* position, int64_t rows, int64_t N, const int32_t* sel, int64_t n_sel,
                                  float* out, hipStream_t s);
hipError_t launch_ppo_gae_p2(const double* rew, const uint8_t* done, const float* val, int T, int64_t N,
                             const int32_t* sel, int64_t n_sel, float gamma, float gamma_lam, float* adv, float* ret,
                             hipStream_t s);

}  // namespace fsk
