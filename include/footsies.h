/*
 * footsies.h -- C-ABI of libfootsies.so, the MI355X-native vectorized FOOTSIES
 * simulator (HIP kernels for gfx950).
 *
 * The reference has no native FFI for this path: its boundary is a Python
 * gymnasium.Env (FootsiesEnv) talking over TCP to a Unity process.  Every entry
 * point below replaces one piece of that stack for N independent arenas at once;
 * the piece is cited next to it (paths relative to the reference root,
 * FE = footsies-gym/footsies_gym/envs/footsies.py, BC = Assets/Script/BattleCore.cs).
 *
 * Conventions
 *   - plain C types only; no exceptions cross the ABI; every call returns 0 on
 *     success or a negative FS_E_* code, with a message via fs_last_error();
 *   - one handle = one device + one HIP stream; calls on a handle must be
 *     serialised by the caller, different handles may run on different threads;
 *   - the library allocates and owns its device buffers; caller buffers are
 *     borrowed for the duration of the call only (unless bound with
 *     fs_bind_outputs, see below);
 *   - fs_step / fs_step_n / fs_reset are asynchronous on the handle's stream;
 *     fs_sync() or the caller's own stream sync orders host reads.
 */
#ifndef FOOTSIES_H
#define FOOTSIES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 8

/* error codes */
#define FS_OK 0
#define FS_E_INVALID (-1)      /* bad argument (FE:100-108 raises ValueError for bad ctor args) */
#define FS_E_DEVICE (-2)       /* HIP runtime failure / no device */
#define FS_E_UNSUPPORTED (-3)  /* configuration not implemented */
#define FS_E_OOM (-4)
#define FS_E_RUNTIME (-5)      /* fs_create found no device and two HIP / HSA runtime images in the process */

/* P2 controller (GameManager.cs:183-190: --p2-bot / remote actor; FE:234-247) */
#define FS_P2_EXTERNAL 0  /* P2 action supplied every step (FE `opponent` callable / remote actor) */
#define FS_P2_BOT 1       /* the in-game scripted BattleAI (BattleAI.cs:10-403) as TrainingBattleAIActor */
#define FS_P2_NOOP 2      /* P2 input always 0 */

/* P1 controller (GameManager.cs:185-200; FE:118, 230-232 `by_example`) */
#define FS_P1_EXTERNAL 0  /* P1 action supplied every step (the agent, TrainingRemoteActor) */
#define FS_P1_BOT 1       /* by_example: the in-game BattleAI plays P1 (--p1-bot --p1-spectator); the
                             agent only observes.  Both bots draw from the game's one UnityEngine.Random,
                             P1 first (TrainingManager.cs:59-77).  The spectator wrapper is not a
                             TrainingBattleAIActor, so P1's BattleAI is never Reset (BC:274-275) */

/* Float evaluation model of the C# arithmetic (parity-unpinned: no Unity binary here) */
#define FS_FLOAT_STRICT32 0  /* every float expression rounded to IEEE binary32 per operation (default) */
#define FS_FLOAT_DOUBLE 1    /* expression temporaries in binary64, rounded to binary32 on store/call */

/* Auto-reset of terminated arenas inside fs_step (the Unity KO->End->Stop->Intro->Fight
 * burst, BC:212-243 / 247-345, which the reference runs without waiting for the agent) */
#define FS_AUTORESET_SAME_STEP 0  /* gymnasium 0.29 SyncVectorEnv: obs = state(-1), final_* = terminal obs */
#define FS_AUTORESET_NEXT_STEP 1  /* gymnasium 1.x: the step after a terminal one runs the burst only */

/* fs_step flags */
#define FS_ACT_HOST 0    /* action pointers are host memory (copied H2D on the handle's stream) */
#define FS_ACT_DEVICE 1  /* action pointers are device memory */

/* fs_reset flags */
#define FS_RESET_HARD 0         /* RESET remote-control command (BC:143-146): Stop->Intro->Fight now */
#define FS_RESET_IF_NEEDED 1    /* FootsiesEnv.reset (FE:482-515): RESET only arenas whose
                                   has_terminated flag is clear; the others just finish the
                                   pending KO->...->Fight burst (if any) and report state(-1) */
#define FS_RESET_SEED_ONLY 2    /* SEED command alone (BC:170-173): Random.InitState on the masked
                                   arenas, nothing else changes and no outputs are written */

#define FS_MAX_FRAME_DELAY 4096

typedef struct fs_config {
  int32_t num_envs;        /* arenas on this handle (>0) */
  int32_t device_id;       /* HIP device ordinal */
  int32_t p2_mode;         /* FS_P2_* */
  int32_t dense_reward;    /* 1: FE._get_dense_reward (FE:388-405, default FE:50); 0: sparse (FE:382-386) */
  int32_t frame_delay;     /* FE:36, 126-131, 493-504, 532-535: observation/info outputs are those of
                              the state frame_delay steps back (d copies of state(-1) after a reset);
                              reward, terminated and fs_get_env_state are the newest state's.
                              0 .. FS_MAX_FRAME_DELAY; the queue takes frame_delay x num_envs x 32 bytes
                              of device memory (8.6 GB at 4096 with 65 536 arenas) */
  int32_t float_mode;      /* FS_FLOAT_* */
  int32_t autoreset_mode;  /* FS_AUTORESET_* */
  int32_t p1_mode;         /* FS_P1_* */
  uint64_t base_seed;      /* arena i's game RNG is seeded with (int32)(base_seed + arena_base + i) at
                              creation (Random.InitState, BC:170-173) */
  uint64_t arena_base;     /* global index of arena 0 when the arenas of one run are sharded over
                              several handles / GPUs: the hashed action stream (fs_step_n,
                              fs_hash_actions), the in-kernel actor's sampling stream and the creation
                              seeds are keyed by the global index, so results do not depend on the
                              sharding.  0 for an unsharded handle */
} fs_config;

/*
 * Per-step outputs, struct-of-arrays, row i = arena i.  Pairs are [N][2]
 * (column 0 = P1, column 1 = P2) exactly like FootsiesEnv's observation tuples
 * (FE:360-368) stacked over arenas.
 */
typedef struct fs_outputs {
  uint8_t* guard;        /* [N][2] obs["guard"]                       (FE:361)              */
  uint8_t* move;         /* [N][2] obs["move"] = FOOTSIES_MOVE_ID_TO_INDEX, DEAD/WIN->STAND (FE:362-365, 537-549) */
  float* move_frame;     /* [N][2] obs["move_frame"], 0 for STAND/FORWARD/BACKWARD (FE:339-358) */
  float* position;       /* [N][2] obs["position"]                    (FE:367)              */
  double* reward;        /* [N]    dense or sparse reward, float64 like FE (FE:382-405)     */
  uint8_t* terminated;   /* [N]    p1Vital==0 or p2Vital==0           (FE:555)              */
  uint8_t* truncated;    /* [N]    always 0                           (FE:569-570)          */
  int32_t* frame;        /* [N]    info["frame"] = globalFrame        (FE:373)              */
  uint8_t* action;       /* [N][2] info["p1_action"/"p2_action"] as 3-bit ints (Left=1, Right=2, Attack=4; state.py:26-36) */
  uint8_t* hitstun;      /* [N][2] info["p1_hitstun"/"p2_hitstun"]   (FE:376-377)          */
  /* FS_AUTORESET_SAME_STEP only: the terminal observation/info of arenas whose
     terminated flag is set this step (other rows are left untouched) */
  uint8_t* final_guard;      /* [N][2] */
  uint8_t* final_move;       /* [N][2] */
  float* final_move_frame;   /* [N][2] */
  float* final_position;     /* [N][2] */
  int32_t* final_frame;      /* [N]    */
  uint8_t* final_action;     /* [N][2] */
  uint8_t* final_hitstun;    /* [N][2] */
} fs_outputs;

/*
 * Raw EnvironmentState of one arena (Assets/Script/EnvironmentState.cs:10-46,
 * built by BattleCore.GetEnvironmentState, BC:449-468).  Used for state-level
 * parity checks and for a wire-compatible JSON server.
 */
typedef struct fs_env_state {
  int32_t p1Vital, p2Vital, p1Guard, p2Guard;
  int32_t p1Move, p1MoveFrame, p2Move, p2MoveFrame;  /* raw actionIDs (0..510) */
  float p1Position, p2Position;
  int32_t globalFrame;
  int32_t p1MostRecentAction, p2MostRecentAction;
  int32_t p1Hitstun, p2Hitstun;
} fs_env_state;

/*
 * Canonical full state of one arena: everything the simulation carries from one
 * frame to the next (Fighter.cs:73-112, BC:56-70, BattleAI.cs:26-32), in a
 * representation-independent form.  Both the HIP path and the CPU oracle export
 * it, so lockstep tests compare hidden state, not only observations.
 */
typedef struct fs_fighter_state {
  float position_x;
  int32_t action_id;            /* raw actionID */
  int32_t action_frame;
  int32_t hit_count;
  int32_t hitstun;
  int32_t vital;
  int32_t guard;
  int32_t buffer_action_id;     /* -1 = none */
  int32_t reserve_action_id;    /* -1 = none */
  uint32_t input_dir_history;   /* Left/Right bits of input[0..15], 2 bits per frame, input[0] in bits 0-1 */
  int32_t attack_hold;          /* consecutive frames input[0..] had Attack, saturating at 63 */
  uint8_t is_input_backward;
  uint8_t is_reserve_proximity_guard;
  uint8_t has_won;
  uint8_t facing_flipped;       /* 0: the player's own facing (P1 right, P2 left: SetupBattleStart, F:124);
                                   1: the other (Fighter.isFaceRight restored by LoadState, F:744) */
  float position_y;             /* Fighter.position.y (F:742): 0 in every state the game reaches by itself;
                                   a loaded y moves every box (TransformToFightRect F:706-719) and is added
                                   to itself by every push (BC:483-519 pass position.y to
                                   ApplyPositionChange, F:331-350) until the next round start (F:123) */
} fs_fighter_state;

typedef struct fs_arena_state {
  fs_fighter_state f[2];
  int32_t frame_count;          /* BattleCore.frameCount */
  int32_t recording_count;      /* currentRecordingInputIndex, saturating at 18000 */
  uint8_t recording_last[2];    /* recordingPnInput[index-1].input */
  uint8_t actor_input[2];       /* TrainingRemoteActor.input of the remote P1 / P2 actors: the last action
                                   received (stale inputs fed to the Intro tick); 0 where that player has no
                                   remote actor (a bot-created P2, FS_P2_NOOP, FS_P1_BOT) */
  uint8_t reset_pending;        /* FS_AUTORESET_NEXT_STEP: terminal, burst not yet run */
  uint8_t has_terminated;       /* FootsiesEnv.has_terminated (FE:191, 508, 563) */
  uint8_t pad0[2];
  double cumulative_reward;     /* FootsiesEnv._cummulative_episode_reward (FE:187) */
  /* The game's UnityEngine.Random (Xorshift128 state).  One per game, shared by both bots; kept and
     seeded in every mode, so a bot switched in later draws from the seeded stream. */
  uint32_t rng[4];
  /* P2's BattleAI (BattleAI.cs:26-32) */
  int32_t move_plan, move_index;     /* moveQueue as (plan id, dequeued count); plan -1 = empty */
  int32_t attack_plan, attack_index; /* attackQueue likewise */
  float prev_distance;          /* BattleAI.fightStates[5] (== previous call's state) */
  int32_t prev_opponent_action; /* raw actionID of the opponent in that FightState */
  /* actors (ABI 2) */
  uint8_t p2_bot;               /* 1: TrainingManager.actorP2 is the bot (FS_P2_BOT handles always; an
                                   FS_P2_EXTERNAL handle after fs_set_p2_mode) */
  uint8_t bot_ready[2];         /* P1 / P2 BattleAI: fightStates[5] is set, i.e. getNextAIInput has run
                                   since construction or Reset (AI:41-47); 0 = its next call returns 0 */
  uint8_t bot_input[2];         /* TrainingBattleAIActor.input of the P1 / P2 bot (its last answer) */
  uint8_t pad1[3];
  /* P1's BattleAI (FS_P1_BOT), fields as P2's */
  int32_t p1_move_plan, p1_move_index;
  int32_t p1_attack_plan, p1_attack_index;
  float p1_prev_distance;
  int32_t p1_prev_opponent_action;
} fs_arena_state;

typedef struct fs_context* fs_handle;

/* Library / ABI version (FS_ABI_VERSION). */
int fs_abi_version(void);

/* The HIP and HSA runtime images mapped into this process, one "hip:<path>" / "hsa:<path>" line
 * each, written NUL-terminated into buf (truncated to len); returns the larger of the two image
 * counts (1 when the process holds one runtime).  fs_create returns FS_E_RUNTIME, naming both
 * paths, when it finds no device and more than one image of either runtime (ABI 7). */
int fs_runtime_images(char* buf, size_t len);

/* Pinned, device-mapped host memory (hipHostMalloc, zero-filled) and its device address, for
 * callers without a device-memory library of their own -- the torch-free Python surface binds its
 * host outputs there (fs_bind_outputs takes *dev); fs_host_free releases it.  fs_memcpy is a
 * synchronous copy between any two addresses the runtime knows (hipMemcpyDefault).  (ABI 7) */
int fs_host_alloc(int device, size_t bytes, void** host, void** dev);
int fs_host_free(void* host);
int fs_memcpy(void* dst, const void* src, size_t bytes);

/* The HIP runtime version the library is bound to (hipRuntimeGetVersion) and the HIP_VERSION it
 * was compiled against, either pointer optional (ABI 7). */
int fs_runtime_version(int* runtime, int* build);

/* Create N arenas on a device and run the game-start sequence (BattleCore.Start
 * + first Stop->Intro->Fight ticks, BC:105-128, 176-200, 262-291) so they sit at
 * state(-1).  Replaces FootsiesEnv.__init__ + _instantiate_game + _connect_to_game
 * (FE:34-290).  Returns FS_E_INVALID for an out-of-range field. */
int fs_create(const fs_config* cfg, fs_handle* out);

/* Reset arenas (FootsiesEnv.reset, FE:482-515).  seeds: optional host array [N]
 * -> Random.InitState((int32)seed) first (SEED command, BC:170-173; FE:487-488);
 * mask: optional host array [N] of 0/1 selecting arenas (NULL = all); flags:
 * FS_RESET_*.  Writes state(-1) observations of the reset arenas into the
 * outputs (reward 0, terminated 0). */
int fs_reset(fs_handle h, const uint64_t* seeds, const uint8_t* mask, int flags);

/* Switch P2 of the masked arenas (host [N] 0/1, NULL = all) between the remote actor
 * (FS_P2_EXTERNAL) and the in-game bot (FS_P2_BOT): the P2_BOT remote-control command
 * (BC:158-167, TrainingRemoteControl.cs:100-102) that FootsiesEnv.set_opponent sends
 * (FE:458-480).  Only for handles created with FS_P2_EXTERNAL -- the reference needs a
 * custom opponent to accept the command (FE:468-470) -- else FS_E_UNSUPPORTED.  The
 * switch applies from the next tick.  The bot keeps its own state while inactive (queues,
 * FightState, last answer), the remote actor its last received action.  Since such a game
 * was launched without --p2-bot, BattleCore's Intro throws before it could Reset the
 * switched-in bot (BC:276-277, GameManager.cs:187), so that bot is never Reset. */
int fs_set_p2_mode(fs_handle h, int mode, const uint8_t* mask);

/* One Fight tick of every arena (FootsiesEnv.step, FE:518-570 -> BC:201-220,
 * 347-364), with auto-reset of terminated arenas per cfg.autoreset_mode.
 * p1_act: [N] 3-bit inputs (Left=1, Right=2, Attack=4; InputData.cs:8-14); ignored (may be
 * NULL) for FS_P1_BOT.
 * p2_act: [N] for FS_P2_EXTERNAL (read for the arenas whose P2 is the remote actor),
 * ignored (may be NULL) otherwise.
 * flags: FS_ACT_HOST or FS_ACT_DEVICE for where the action arrays live. */
int fs_step(fs_handle h, const uint8_t* p1_act, const uint8_t* p2_act, int flags);

/* fs_step for the arenas whose active[i] != 0 only; the others keep their state
 * and their outputs (which then still hold their previous step's values).  This
 * lets arenas advance at their own pace, as N separate FootsiesEnv instances do
 * under a frame-skipping wrapper (wrappers/frame_skip.py:63-80).  active lives
 * where flags says the actions do.  With frame_delay > 0 each arena's delayed-frame
 * queue advances with that arena's own steps (every FootsiesEnv keeps its own deque). */
int fs_step_masked(fs_handle h, const uint8_t* p1_act, const uint8_t* p2_act, const uint8_t* active, int flags);

/* One agent decision per arena under the reference's frame-skip wrapper
 * (wrappers/frame_skip.py:46-80), in one kernel launch: each active arena runs the tick that
 * takes p1_act[i], then keeps ticking with input 0 while its own observation is skippable --
 * P1's observed move_frame != 0 and P2's observed move none of DAMAGE / GUARD_STAND /
 * GUARD_CROUCH / GUARD_M / GUARD_BREAK, or P1's observed move DAMAGE (frame_skip.py:49-61) --
 * and the episode goes on, at most max_ticks ticks in this call.  Every tick is fs_step's
 * (auto-reset burst, final_* records, the bot, the cumulative reward); the rewards are summed in
 * float64 in tick order from 0.0, as frame_skip.py:71-78 sums them.  Afterwards the handle's
 * regular or bound outputs hold each active arena's last tick with `reward` set to the sum; in
 * FS_AUTORESET_SAME_STEP final_* holds the terminal record of an arena that ended.  A
 * FS_AUTORESET_NEXT_STEP arena with a reset pending runs the reset burst alone (state(-1), reward
 * 0: never skippable).
 *   active: [N] 0/1 or NULL (all arenas), living where flags says the actions live.  Inactive arenas
 *     keep their state, outputs, accumulators and their ticks / pending entries (fs_step_masked).
 *   flags: FS_ACT_HOST or FS_ACT_DEVICE, optionally | FS_SKIP_RESUME.  Without FS_SKIP_RESUME p1_act
 *     is required and a new decision starts for the active arenas.  With it p1_act is ignored (may
 *     be NULL) and the active arenas continue their decision with input 0 from the handle's
 *     accumulators: a caller loops
 *       fs_step_skip(h, NULL, out.pending, FS_ACT_DEVICE | FS_SKIP_RESUME, cap, &out)
 *     until n_pending is 0.  Any split into caps gives results bit-identical to one uncapped call,
 *     the reward sum and final_* included.
 *   out: optional device arrays, each optional.
 * fs_steps_taken advances by 1 per call (as fs_step_masked).  Asynchronous on the handle's stream.
 * FS_E_UNSUPPORTED for a handle created with FS_P2_EXTERNAL (a remote P2 must answer every frame;
 * also after fs_set_p2_mode), for FS_P1_BOT, and with frame_delay > 0 (the delayed queue consumes
 * every tick's row).  FS_E_INVALID for max_ticks < 1, a missing p1_act without FS_SKIP_RESUME, or
 * unknown flag bits.  (ABI 8) */
#define FS_SKIP_RESUME 2   /* or'd into flags beside FS_ACT_HOST / FS_ACT_DEVICE */
#define FS_SKIP_DEFAULT_MAX_TICKS 64
typedef struct fs_skip_out {
  int32_t* ticks;      /* [N] device, optional: ticks this arena ran for the current decision (all resumes included) */
  uint8_t* pending;    /* [N] device, optional: 1 = still skippable at the cap; may alias `active` */
  int32_t* n_pending;  /* [1] device, optional: set (not added) to the number of pending arenas of this call */
} fs_skip_out;
int fs_step_skip(fs_handle h, const uint8_t* p1_act, const uint8_t* active, int flags, int max_ticks,
                 const fs_skip_out* out);

/* n Fight ticks in one kernel launch (fused rollout).  Actions: device arrays
 * [n][N], or NULL to draw them on device from the counter-based hash
 * a = splitmix64(action_seed ^ env*0x9E3779B97F4A7C15 ^ (t << 1 | player)) & 7
 * with env = cfg.arena_base + i and t = fs_steps_taken(h) + k.  traj: device arrays laid out [n][N] (pairs
 * [n][N][2]) receiving every tick's outputs; traj == NULL writes each tick
 * into the handle's regular outputs (the last tick remains visible; with
 * frame_delay > 0 the n ticks are then launched one by one, since the delayed
 * queue consumes every tick's row).  Trajectory rows are addressed with 32-bit
 * byte offsets, so a call with n * N above 2^29 - 1 arena-ticks runs as several
 * consecutive launches over row ranges of the same buffers, with identical
 * results. */
int fs_step_n(fs_handle h, int n, const uint8_t* p1_act, const uint8_t* p2_act,
              uint64_t action_seed, const fs_outputs* traj);

/* A packed trajectory for fs_step_n_packed: the values of an fs_outputs trajectory in two
 * stores per tick instead of ten.  Row r = t * N + i (tick t, arena i); k = 0 (P1), 1 (P2):
 *   lanes[r][k]: 16 bytes -- byte 0 guard, 1 move, 2 action (3-bit MostRecentAction), 3 hitstun;
 *                bytes 4-7 move_frame (float), 8-11 position (float); bytes 12-15: for k = 0 the
 *                frame (int32), for k = 1 byte 12 terminated, byte 13 truncated, bytes 14-15 zero.
 *   reward[r]:   float64, as fs_outputs.reward.
 *   final_lanes[r][k] (FS_AUTORESET_SAME_STEP; rows of arenas that did not end are left
 *                untouched): the terminal record in the lanes layout, bytes 12-15 of k = 0 the
 *                final frame, of k = 1 zero.
 * lanes and final_lanes must be 16-byte aligned.  Every field equals the corresponding
 * fs_outputs trajectory field of fs_step_n on the same state and actions. */
#define FS_PACKED_LANE_BYTES 16
typedef struct fs_packed_traj {
  void* lanes;        /* [n][N][2][16 B] */
  double* reward;     /* [n][N] */
  void* final_lanes;  /* [n][N][2][16 B]; required in FS_AUTORESET_SAME_STEP */
} fs_packed_traj;

/* fs_step_n with action rows (p1_act required; p2_act as for fs_step_n) into a packed trajectory.
 * FS_E_UNSUPPORTED with frame_delay > 0. */
int fs_step_n_packed(fs_handle h, int n, const uint8_t* p1_act, const uint8_t* p2_act, const fs_packed_traj* traj);

/* The actor of fs_step_n_policy: an MLP 8 -> 64 -> tanh -> 64 -> tanh -> 8 on
 * P1's observation features [guard/3, move/16, move_frame/55, position/4.6] of
 * P1 then P2 (footsies_gym_amd/rollout.py obs_features), fp32 device weights in
 * torch nn.Linear layouts (weight [out][in]), computed in bf16 with f32
 * accumulation.  The action is drawn from softmax(logits) by inverse CDF with
 * u = uniform(seed, env, t) (fs_policy.h policy_uniform), t = fs_steps_taken + k.
 * For finite logits the draw is never an action whose softmax weight underflowed
 * to exactly zero in float32 (a logit more than ~87 below the largest). */
typedef struct fs_policy {
  const float* w1; /* [64][8] */
  const float* b1; /* [64] */
  const float* w2; /* [64][64] */
  const float* b2; /* [64] */
  const float* w3; /* [8][64] */
  const float* b3; /* [8] */
  uint64_t seed;
  uint8_t* actions_out; /* [n][N] device: P1's sampled actions, or NULL */
  float* logp_out;      /* [n][N] device: their log-probabilities, or NULL */
} fs_policy;

/* fs_step_n with P1 driven by the actor `pol` inside the fused tick loop: the
 * whole policy-in-the-loop rollout in one launch.  p2_act:
 * device [n][N] for FS_P2_EXTERNAL, ignored otherwise.  traj as in fs_step_n.
 * FS_E_UNSUPPORTED with frame_delay > 0. */
int fs_step_n_policy(fs_handle h, int n, const fs_policy* pol, const uint8_t* p2_act, const fs_outputs* traj);

/* n agent decisions per arena in one kernel launch: fs_step_n_policy's actor in front of
 * fs_step_skip's loop, i.e. a policy rollout under the reference's frame-skip wrapper
 * (wrappers/frame_skip.py:46-80).  For decision d = 0 .. n-1 of arena i the actor sees the arena's
 * observation as it stands (the handle's state at the call for d = 0, then the last tick's), draws
 * the action with u = uniform(pol->seed, cfg.arena_base + i, fs_steps_taken + d), and the arena
 * runs the tick that takes it, then ticks with input 0 while its observation is skippable
 * (fs_step_skip's test) and the episode goes on.  Every tick is fs_step's.  Arenas skip their own
 * number of ticks, and every output is indexed by decision: row d * N + i of traj receives the
 * decision's last tick with `reward` set to the float64 sum of its ticks' rewards in tick order
 * from 0.0 (FS_AUTORESET_SAME_STEP: final_* the terminal record of a decision that ended the
 * episode); pol->actions_out / pol->logp_out are [n][N] per decision.  A FS_AUTORESET_NEXT_STEP
 * arena with a reset pending runs the reset burst alone: its sampled action is recorded and
 * ignored, ticks = 1, reward = 0.
 *   max_ticks (1 .. FS_SKIP_POLICY_MAX_TICKS) closes a decision: an arena still skippable after
 *     that many ticks ends the decision there (capped = 1) and its next decision is an ordinary
 *     one, so every arena is at a decision boundary when the call returns, nothing but the arena
 *     state carries over between calls, and a call runs at most n * max_ticks ticks.  Whenever
 *     no decision is capped the results are the reference wrapper's on the same actions.
 *   traj: as in fs_step_n (NULL: the handle's regular or bound outputs hold the last decision).
 *   skip: optional, each array optional.
 * fs_steps_taken advances by n.  Asynchronous on the handle's stream.  n * N above the
 * trajectory row limit runs as consecutive launches (every launch ends on decision boundaries:
 * identical results).  FS_E_UNSUPPORTED where fs_step_skip returns it (FS_P2_EXTERNAL handles,
 * FS_P1_BOT, frame_delay > 0); FS_E_INVALID for n < 1, max_ticks out of range, a NULL pol or
 * weight array.  (ABI 8: an addition) */
#define FS_SKIP_POLICY_MAX_TICKS 4096
typedef struct fs_skip_traj {
  int32_t* ticks;   /* [n][N] device, optional: ticks each decision ran */
  uint8_t* capped;  /* [n][N] device, optional: 1 = closed at max_ticks while still skippable */
} fs_skip_traj;
int fs_step_skip_policy(fs_handle h, int n, const fs_policy* pol, int max_ticks,
                        const fs_outputs* traj, const fs_skip_traj* skip);

/* Self-play in one launch: fs_step_n_policy with a second in-kernel actor playing P2, so the
 * opponent reacts to the game every tick (the reference's custom `opponent` policy, FE:47, 119,
 * 525-527, on the fused path).  Every tick is fs_step's with P1's input sampled from p1 and P2's
 * from p2; reward, traj and the regular outputs are fs_step_n_policy's (the reward is P1's).
 *   p1, p2: both actors in full (six weight arrays each).  p2->seed is P2's own sampling seed:
 *     u = uniform(p2->seed, cfg.arena_base + i, fs_steps_taken + k), the function and counter of
 *     P1's draw.  p2->actions_out / p2->logp_out ([n][N] device, optional) receive P2's sampled
 *     index -- before the Left/Right exchange below -- and its log-probability.
 *   flags = 0: P2's actor sees P1's observation (g1, g2, m1, m2, mf1, mf2, x1, x2), which is what
 *     the reference hands `opponent(obs, info)` (FE:526), and its sampled index is P2's input.
 *   flags = FS_SELFPLAY_MIRROR: P2's actor sees the game from its own side -- each feature pair
 *     swapped and both positions negated (g2, g1, m2, m1, mf2, mf1, -x2, -x1) -- and P2's input is
 *     its sampled index a with Left (1) and Right (2) exchanged, (a & 4) | ((a & 1) << 1) |
 *     ((a >> 1) & 1): one set of weights plays either side.
 * fs_steps_taken advances by n.  Asynchronous on the handle's stream; n * N above the trajectory
 * row limit runs as consecutive launches with identical results.  FS_E_UNSUPPORTED unless the
 * handle's P2 is FS_P2_EXTERNAL with no arena switched to the bot (fs_set_p2_mode), P1 is the agent
 * and frame_delay is 0; FS_E_INVALID for n <= 0, unknown flag bits, a NULL actor or weight array,
 * or trajectory buffers fs_step_n_policy would refuse.  (ABI 8: an addition) */
#define FS_SELFPLAY_MIRROR 1
int fs_step_n_selfplay(fs_handle h, int n, const fs_policy* p1, const fs_policy* p2, int flags,
                       const fs_outputs* traj);

/* Self-play per agent decision in one launch: fs_step_skip_policy with fs_step_n_selfplay's second
 * actor, i.e. the reference's FootsiesFrameSkipped over a FootsiesEnv with a custom `opponent`
 * (wrappers/frame_skip.py:65-80 calls env.step once per tick, and FE:525-527 asks `opponent`
 * inside every env.step).  P1's actor decides once per decision -- the tick that takes its action,
 * then input 0 while the arena's observation is skippable and the episode goes on, exactly as in
 * fs_step_skip_policy -- and P2's actor acts on every tick, the ticks P1 skips included, on the
 * observation as it stands before that tick.  flags: 0 or FS_SELFPLAY_MIRROR, as in
 * fs_step_n_selfplay.  Draws, for arena i's decision d (counter c = fs_steps_taken + d):
 *   P1: u = uniform(p1->seed, cfg.arena_base + i, c), fs_step_skip_policy's;
 *   P2 on tick j of the decision: u = uniform(p2->seed, cfg.arena_base + i, c + ((uint64_t)j << 40)),
 * so results depend neither on how a call is split nor on the other arenas, and with max_ticks = 1
 * the call is fs_step_n_selfplay bit for bit.
 *   traj, skip->ticks, skip->capped, p1->actions_out, p1->logp_out: by decision, as in
 *     fs_step_skip_policy (the row is the decision's last tick, `reward` the float64 sum of its
 *     ticks' rewards in tick order from 0.0; a FS_AUTORESET_NEXT_STEP arena with a reset pending
 *     runs the reset burst alone, ticks = 1, reward = 0, both samples recorded and ignored).
 *   p2->actions_out / p2->logp_out: optional, device [n][max_ticks][N]: entry (d, j, i) is P2's
 *     sampled index (before the Left/Right exchange) and its log-probability on tick j of arena i's
 *     decision d; entries of ticks that did not run are left untouched.  For tests and diagnostics.
 * fs_steps_taken advances by n.  Asynchronous on the handle's stream; n * N above the trajectory
 * row limit runs as consecutive launches that end on decision boundaries (identical results).
 * FS_E_UNSUPPORTED where fs_step_n_selfplay returns it; FS_E_INVALID for n < 1, max_ticks outside
 * 1 .. FS_SKIP_POLICY_MAX_TICKS, unknown flag bits, a NULL actor or weight array, fs_steps_taken +
 * n >= 2^40 (P2's counter would repeat), or n * max_ticks * N above INT32_MAX when a P2 array is
 * given.  (ABI 8: an addition) */
int fs_step_skip_selfplay(fs_handle h, int n, const fs_policy* p1, const fs_policy* p2, int flags,
                          int max_ticks, const fs_outputs* traj, const fs_skip_traj* skip);

/* The C5 learner (footsies_gym_amd/ppo.py, PPOTrainer(learner="hip")): an MLP
 * 8 -> 64 -> tanh -> 64 -> tanh -> out, fp32 device weights in torch nn.Linear layouts. */
typedef struct fs_mlp {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
} fs_mlp;
#define FS_PPO_ACTOR_PARAMS 5256  /* w1 512, b1 64, w2 4096, b2 64, w3 512, b3 8 */
#define FS_PPO_CRITIC_PARAMS 4801 /* w1 512, b1 64, w2 4096, b2 64, w3 64, b3 1 */

/* Self-play against a pool of opponents in one launch: fs_step_n_selfplay / fs_step_skip_selfplay with
 * P2's weights chosen per group of FS_SELFPLAY_GROUP consecutive arenas (local index i, group i / 128;
 * the last group may be partial) from `n_slots` actors held in one device buffer.  Group g plays slot
 * min(slot[g], n_slots - 1): no value of a slot byte reads outside the pool.  Nothing else differs --
 * P1's actor, both seeds and draw counters, the flags, traj / skip and the sample arrays are those of the
 * call each one extends -- so arena i's results are bit for bit those of fs_step_n_selfplay (or
 * fs_step_skip_selfplay) with p2 set to the six arrays of slot[i / 128], p2->seed = pool->seed and the same
 * output arrays.  Split launches (n * N above the trajectory row limit) offset the sample arrays as those
 * calls do; `slot` is per group and is read whole by every launch.
 * Returns what the extended call returns (FS_E_UNSUPPORTED on the same handles; FS_E_INVALID for the same
 * n, flags, max_ticks, 2^40 and int32 bounds, pool->actions_out / logp_out standing for p2's), and
 * FS_E_INVALID for a NULL pool, weights or slot or n_slots outside 1 .. FS_SELFPLAY_POOL_MAX.
 * (ABI 8: an addition) */
#define FS_SELFPLAY_GROUP 128      /* arenas i with equal i / 128 share an opponent */
#define FS_SELFPLAY_POOL_MAX 256
typedef struct fs_policy_pool {
  const float* weights;   /* [n_slots][FS_PPO_ACTOR_PARAMS] device, fp32, slot = w1|b1|w2|b2|w3|b3 */
  int n_slots;            /* 1 .. FS_SELFPLAY_POOL_MAX */
  const uint8_t* slot;    /* [ceil(N / FS_SELFPLAY_GROUP)] device: each group's slot */
  uint64_t seed;          /* P2's sampling seed, as fs_policy.seed */
  uint8_t* actions_out;   /* as p2->actions_out of the call it extends */
  float* logp_out;
} fs_policy_pool;
int fs_step_n_selfplay_pool(fs_handle h, int n, const fs_policy* p1, const fs_policy_pool* pool, int flags,
                            const fs_outputs* traj);
int fs_step_skip_selfplay_pool(fs_handle h, int n, const fs_policy* p1, const fs_policy_pool* pool, int flags,
                               int max_ticks, const fs_outputs* traj, const fs_skip_traj* skip);

/* Self-play leagues: the two pool calls on a handle where chosen groups play the in-game bot.  The handle's
 * P2 bit (fs_set_p2_mode) says who plays a group of FS_SELFPLAY_GROUP consecutive arenas (the last, partial
 * one counts as a group) and may change between calls; within a group it must be uniform.
 *   A remote group is that group of fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool bit for bit: P2's
 *     weights from slot[g], the draws
 *       P1: u = uniform(p1->seed, cfg.arena_base + i, c), c = fs_steps_taken + k (tick or decision k),
 *       P2: u = uniform(pool->seed, cfg.arena_base + i, c) per tick, or c + ((uint64_t)j << 40) on tick j of
 *           a decision,
 *     flags (0 or FS_SELFPLAY_MIRROR) and both actors' sample arrays as in those calls.
 *   A bot group is fs_step_n_policy on such arenas: P1's actor, with the same seed, draw function and counter
 *     c, against the arena's BattleAI, with the switch's semantics of fs_set_p2_mode (the switched-in bot is
 *     never Reset, P2's remote input goes stale, the game RNG advances as in fs_step).  No P2 actor runs:
 *     slot[g] is ignored and the entries of pool->actions_out / logp_out that belong to these arenas are left
 *     untouched.  In fs_step_skip_league P1 decides once per decision and the bot acts on every tick; the
 *     outputs are by decision as fs_step_skip_selfplay defines them (the last tick's row, the float64 reward
 *     sum from 0.0 in tick order, skip->ticks, skip->capped).
 * With no arena switched the calls are the pool calls bit for bit; fs_step_skip_league with max_ticks = 1 is
 * fs_step_n_league.  Arguments, launch split and return codes are the pool calls', except that switched
 * arenas are accepted: FS_E_UNSUPPORTED (the message names the first such group) only for a group with
 * both kinds of P2, and as before unless the handle's P2 is FS_P2_EXTERNAL, P1 the agent and frame_delay 0.
 * The four calls above keep refusing a handle with any arena switched.  (ABI 8: an addition) */
int fs_step_n_league(fs_handle h, int n, const fs_policy* p1, const fs_policy_pool* pool, int flags,
                     const fs_outputs* traj);
int fs_step_skip_league(fs_handle h, int n, const fs_policy* p1, const fs_policy_pool* pool, int flags,
                        int max_ticks, const fs_outputs* traj, const fs_skip_traj* skip);
/* Device workspace fs_ppo_grad needs (independent of n). */
size_t fs_ppo_workspace_bytes(void);
/* One minibatch's gradient of PPO's loss, in fp32 on `stream` (a hipStream_t, NULL =
 * the null stream), asynchronously.  rows: device [n][12] f32 = features[8], action,
 * old log-probability, advantage, return.  The loss is ppo.py's:
 *   -mean(min(r A, clamp(r, 1 - clip, 1 + clip) A)) + vf_coef mean((v - R)^2)
 *   - ent_coef mean(H(softmax(actor(x)))),  r = exp(log p(action) - old),
 * actor with 8 outputs (logits), critic with 1 (v).  grad_out: device
 * [FS_PPO_ACTOR_PARAMS + FS_PPO_CRITIC_PARAMS] f32, each network's gradient in torch
 * parameters() order (w1, b1, w2, b2, w3, b3), as autograd defines it (torch.min
 * splits a tie's gradient, clamp passes it inside its closed range); loss_out: device
 * [3] f32 = the three means (policy, value, entropy).  Summation order is fixed, so
 * repeated calls give identical results. */
/* The update's forward passes without gradient, fp32, asynchronously on `stream`: for
 * x = device [n_values][8] f32 features, values_out[i] = critic(x[i]) for i < n_values, and
 * logp_out[i] = log_softmax(actor(x[i]))[actions[i]] for i < n_logp <= n_values (actions:
 * device uint8 [n_logp]).  Either output may be NULL (its network is then not run). */
int fs_ppo_eval(const float* x, int64_t n_values, const uint8_t* actions, int64_t n_logp, const fs_mlp* actor,
                const fs_mlp* critic, float* values_out, float* logp_out, void* stream);
int fs_ppo_grad(const float* rows, int64_t n, const fs_mlp* actor, const fs_mlp* critic, float clip,
                float vf_coef, float ent_coef, float* grad_out, float* loss_out, void* workspace,
                size_t workspace_bytes, void* stream);
/* The same two calls with the precision of the three 64-wide products (layer 2's forward pass,
 * the backward pass through W2 and dW2) chosen: FS_PPO_FP32 (fs_ppo_grad / fs_ppo_eval: fp32
 * MFMA, exact fp32 products) or FS_PPO_SPLIT_BF16 (each fp32 operand split into a bf16 hi + lo
 * pair and the product taken as hi.hi + hi.lo + lo.hi on bf16 MFMA with fp32 accumulation:
 * relative error per product below 2^-15, ~5x less matrix-pipe time).  The layers with 8 inputs
 * or outputs stay fp32; FS_PPO_SPLIT_BF16 takes tanh and exp from the hardware exp2 / reciprocal
 * (tanh within 2.5e-7 absolutely).  fs_ppo_eval_ex needs the workspace for FS_PPO_SPLIT_BF16 (NULL / 0
 * for FS_PPO_FP32); a workspace is not shared between calls in flight on different streams. */
#define FS_PPO_FP32 0
#define FS_PPO_SPLIT_BF16 1
int fs_ppo_grad_ex(const float* rows, int64_t n, const fs_mlp* actor, const fs_mlp* critic, float clip,
                   float vf_coef, float ent_coef, float* grad_out, float* loss_out, void* workspace,
                   size_t workspace_bytes, void* stream, int precision);
int fs_ppo_eval_ex(const float* x, int64_t n_values, const uint8_t* actions, int64_t n_logp, const fs_mlp* actor,
                   const fs_mlp* critic, float* values_out, float* logp_out, void* workspace, size_t workspace_bytes,
                   void* stream, int precision);
/* fs_ppo_grad_ex over a minibatch of whole runs of the [n_rows][12] table, without gathering it
 * first (ppo.py PPOTrainer.update: runs of consecutive samples in a shuffled order): sample i of
 * the minibatch is row runs[i >> run_shift] * 2^run_shift + (i mod 2^run_shift), for
 * i < n_runs * 2^run_shift; runs: device int64 [n_runs].  Same results, bit for bit, as
 * fs_ppo_grad_ex on those rows gathered in that order.  A run entry whose rows fall outside the
 * table is read as a padding row (nothing read, nothing added; the mean still counts it): the
 * entries are device data, so they are not checked on the host.  (ABI 6.) */
int fs_ppo_grad_runs(const float* rows, int64_t n_rows, const int64_t* runs, int64_t n_runs, int run_shift,
                     const fs_mlp* actor, const fs_mlp* critic, float clip, float vf_coef, float ent_coef,
                     float* grad_out, float* loss_out, void* workspace, size_t workspace_bytes, void* stream,
                     int precision);
/* GAE of a [T][N] trajectory (ppo.py gae), asynchronously on `stream`: rewards device
 * [T][N] f64 and done device [T][N] u8 as fs_step_n_policy's trajectory holds them, values
 * device [T + 1][N] f32 (the last row bootstraps); delta = (r + (gamma v[t+1]) keep) - v[t],
 * keep = 1 - done, adv[t] = delta[t] + gamma_lam keep[t] adv[t + 1] (one fused multiply-add),
 * ret = adv + v[t].  gamma and gamma_lam (= gamma * lam) as the f32 values torch rounds them to. */
int fs_ppo_gae(const double* rewards, const uint8_t* done, const float* values, int T, int64_t N, float gamma,
               float gamma_lam, float* adv_out, float* ret_out, void* stream);
/* The learner's features of n observations, asynchronously on `stream`: out device [n][8] f32
 * (16-byte aligned) = guard / 3, move / 16, move_frame / 55, position / 4.6 of both fighters
 * (wrappers/normalization.py's constants), each x * f32(1 / divisor in f64) as torch computes it; inputs are
 * trajectory columns ([n][2] u8, u8, f32, f32). */
int fs_ppo_features(const uint8_t* guard, const uint8_t* move, const float* move_frame, const float* position,
                    int64_t n, float* out, void* stream);
/* fs_ppo_grad's [n][12] row table from its columns, asynchronously on `stream`: x device
 * [n][8] f32 (16-byte aligned), actions u8 [n], old log-probs, advantages and returns f32 [n],
 * stats device [2] f32 = (mean, std) of the advantages; row = x, action,
 * old, (adv - mean) / (std + 1e-8), ret. */
int fs_ppo_pack(const float* x, const uint8_t* actions, const float* old_logp, const float* adv, const float* ret,
                const float* stats, int64_t n, float* rows_out, void* stream);
/* P2's side of a mirrored self-play trajectory (fs_step_n_selfplay and its pool / league forms under
 * FS_SELFPLAY_MIRROR), for a learner that uses both fighters' samples; asynchronously on `stream`.  (Additions
 * within ABI 8: no existing struct or call changed.)
 *   P2's observation before tick t is the mirror of P1's feature row: each pair swapped and both positions
 * negated, g2, g1, m2, m1, mf2, mf1, -x2, -x1 -- what the in-kernel P2 actor sees.  Its action is its sampled
 * index as fs_policy.actions_out holds it (before Left and Right are exchanged for the game), its old
 * log-probability fs_policy.logp_out.  Its reward is P1's negated: the game is treated as zero-sum, which is
 * exact in f64 for the dense and the sparse reward alike (the dense terms and the terminal correction +-1 - cum
 * negate exactly).  It is FootsiesEnv's reward seen from P2's chair except on a double KO, which FootsiesEnv
 * scores as a P1 win (p2Vital == 0): P2 is then scored a loss, not a win; the outputs carry no vitals, so the
 * two cannot be told apart here.  Its done flag is P1's `terminated`.
 *   `sel`: device int32 [n_sel], the arenas whose P2 samples are wanted, in any order, repeats allowed (runs of
 * consecutive arenas keep the loads coalesced); NULL is the identity 0 .. N - 1 and needs n_sel == N.  The
 * entries are device data and are not checked on the host: one outside [0, N) reads nothing, and its outputs
 * are zeros.
 *   fs_ppo_features_p2: guard, move, move_frame, position are [rows][N][2] trajectory columns; out device
 * [rows][n_sel][8] f32 (16-byte aligned), out[r][c] = the mirrored row of fs_ppo_features' row of (r, sel[c]),
 * bit for bit rollout.py's mirror_features(obs_features(...)) (the negation a sign flip: -0.0 from 0.0).
 *   fs_ppo_gae_p2: fs_ppo_gae on the rewards negated and the rewards and done flags ([T][N]) gathered by sel;
 * values device [T + 1][n_sel] f32, adv_out and ret_out [T][n_sel] f32; bit for bit fs_ppo_gae on those
 * arrays gathered first. */
int fs_ppo_features_p2(const uint8_t* guard, const uint8_t* move, const float* move_frame, const float* position,
                       int64_t rows, int64_t N, const int32_t* sel, int64_t n_sel, float* out, void* stream);
int fs_ppo_gae_p2(const double* rewards, const uint8_t* done, const float* values, int T, int64_t N,
                  const int32_t* sel, int64_t n_sel, float gamma, float gamma_lam,
                  float* adv_out, float* ret_out, void* stream);

/* Fill device arrays p1_out/p2_out [n_steps][N] with the synthetic action stream
 * of fs_step_n (splitmix64 hash of (seed, arena_base + i, t0 + k, player)),
 * so benchmark inputs are resident in HBM before the timed region.
 * p2_out may be NULL. */
int fs_hash_actions(fs_handle h, int n_steps, uint64_t seed, uint64_t t0, uint8_t* p1_out, uint8_t* p2_out);

/* Device pointers of the current outputs, valid until the next call on h. */
int fs_outputs_get(fs_handle h, fs_outputs* out);

/* The host arrays of one FootsiesVectorEnv numpy step (vector_env.step_result_from_outputs, the
 * batched form of FE:336-380's _extract_obs / _extract_info and FE:555-570), in the reference's
 * dtypes: Gymnasium's MultiDiscrete as int64, Box as float32, bools as 0 / 1 bytes.  Any member
 * may be NULL (not written).  [N][2] arrays are P1, P2 per row; *_action are [N][3] (Left, Right,
 * Attack; state.py:26-36). */
typedef struct fs_host_arrays {
  int64_t* guard;            /* obs["guard"]      [N][2] */
  int64_t* move;             /* obs["move"]       [N][2] */
  float* move_frame;         /* obs["move_frame"] [N][2] */
  float* position;           /* obs["position"]   [N][2] */
  int64_t* info_guard;       /* the info's copies of the observation (FE:379) */
  int64_t* info_move;
  float* info_move_frame;
  float* info_position;
  int64_t* frame;            /* info["frame"]      [N] */
  uint8_t* p1_action;        /* info["p1_action"]  [N][3] bool */
  uint8_t* p2_action;        /* info["p2_action"]  [N][3] bool */
  int64_t* p1_hitstun;       /* info["p1_hitstun"] [N] */
  int64_t* p2_hitstun;       /* info["p2_hitstun"] [N] */
  double* reward;            /* [N] */
  uint8_t* terminated;       /* [N] bool */
  uint8_t* truncated;        /* [N] bool */
} fs_host_arrays;

/* Convert host copies of step outputs (`src`: the fs_outputs layout in host memory, e.g. the
 * pinned copy of fs_outputs_get's buffers, `n_src` rows each; only its first ten members are
 * read) into `dst`, over `threads` host threads (a pool kept by the library).  Row i of dst is
 * row rows[i] of src (rows NULL: row i), for i < n -- so the terminal records of the arenas that
 * ended a step are converted by passing the final_* arrays as src's first members and the
 * terminated rows.  FS_E_INVALID (nothing written) when a row index is outside [0, n_src) or,
 * without rows, n > n_src.  (ABI 5 added n_src.) */
int fs_host_convert(const fs_outputs* src, int64_t n_src, const int64_t* rows, int64_t n, const fs_host_arrays* dst,
                    int threads);
/* fs_host_convert started on the library's own threads, returning once its arguments are checked
 * (the same checks and errors); fs_host_convert_wait returns when it has finished.  The caller
 * goes on meanwhile -- FootsiesVectorEnv.step builds the terminated arenas' final-observation
 * dicts (Python, holding the GIL) while the step's arrays are converted -- and keeps src, rows and
 * dst valid until the wait.  One conversion in flight per process: a start while another (another
 * thread's) is in flight waits for it first; a wait returns once none is in flight.  fs_host_convert
 * calls for fewer than 8192 rows run on the calling thread and may overlap it.  (ABI 6.) */
int fs_host_convert_start(const fs_outputs* src, int64_t n_src, const int64_t* rows, int64_t n,
                          const fs_host_arrays* dst, int threads);
int fs_host_convert_wait(void);

/* Pack the current outputs into one FS_RECORD_BYTES record per arena at dst (device,
 * [N][40] bytes): guard[2] move[2] action[2] hitstun[2] u8, terminated u8, truncated
 * u8, pad[2], move_frame[2] f32, position[2] f32, frame i32, reward f64 -- the payload
 * of the multi-GPU per-step gather over RCCL.  Asynchronous. */
#define FS_RECORD_BYTES 40
int fs_pack_outputs(fs_handle h, void* dst);
/* fs_step that also writes every arena's FS_RECORD_BYTES record (fs_pack_outputs' layout) to rec
 * (device, [N][40] bytes, 8-byte aligned) from inside the tick's own kernel: the same bytes as
 * fs_step followed by fs_pack_outputs(h, rec), one launch instead of two -- the per-step gather
 * path of SURVEY.md 8(e).  With frame_delay > 0 (the delayed queue rewrites the outputs after the
 * tick) it is exactly those two calls.  Asynchronous.  (ABI 6.) */
int fs_step_rec(fs_handle h, const uint8_t* p1_act, const uint8_t* p2_act, int flags, void* rec);

/* Redirect the per-step outputs into caller-owned device buffers (e.g. torch
 * tensors) for zero-copy; NULL members keep the library's own buffer.  The
 * buffers must stay alive until fs_destroy or the next bind. */
int fs_bind_outputs(fs_handle h, const fs_outputs* dev);

/* Copy the raw EnvironmentState [N] / canonical full state [N] of every arena
 * to host memory (synchronous).  fs_get_state replaces STATE_SAVE
 * (BC:148-151, 667-674) in canonical form. */
int fs_get_env_state(fs_handle h, fs_env_state* host_out);
int fs_get_state(fs_handle h, fs_arena_state* host_out);
/* Load canonical state [N] from host (STATE_LOAD, BC:153-156, 676-683).
 * Input history beyond what fs_arena_state carries is not representable.  Fighters with
 * position_y != 0 or facing_flipped switch the handle's steps to the kernels' general-geometry
 * path (box y extents tested, y carried through the pushes) until the next fs_set_state loads
 * only standard fighters.
 * FS_E_INVALID (nothing loaded) for a field outside the packed layout's range, or, with the
 * bot as P2, a queue index at or past its plan's length (such a queue is empty: plan -1). */
int fs_set_state(fs_handle h, const fs_arena_state* host_in);

/* Block until all work on the handle's stream is done. */
int fs_sync(fs_handle h);
/* The handle's hipStream_t (as void*), for event timing / torch.cuda.ExternalStream. */
void* fs_stream(fs_handle h);
/* Run all further work of h on a caller-owned hipStream_t (e.g. PyTorch's current
 * stream; NULL = the HIP null stream) instead of the library's own, so device
 * actions/outputs are ordered with the caller's kernels without events.
 * FS_STREAM_OWN restores the library's stream.  The caller keeps the stream
 * alive while h uses it; switching orders the new stream after the old one. */
#define FS_STREAM_OWN ((void*)(intptr_t)-1)
int fs_set_stream(fs_handle h, void* stream);
int fs_num_envs(fs_handle h);
/* Steps (ticks, or decisions of the skip calls) taken so far: the counter of every in-kernel draw.  0 at
 * fs_create, unless the test hook FOOTSIES_STEPS_START (a uint64, decimal or 0x hex) starts it elsewhere. */
uint64_t fs_steps_taken(fs_handle h);
/* The kernel a step call on h would launch, as rocprofv3 names it ("fsk::k_step_n<0, 0>"):
 * n_steps = 1 is fs_step / fs_step_masked, n_steps > 1 fs_step_n with action rows (its launches
 * pick the one-lane kernel from 2 x 64 x SIMD-count arenas on, FOOTSIES_FUSED_LANES forces
 * either); flags FS_KERNEL_HASHED = fs_step_n without action rows, FS_KERNEL_POLICY =
 * fs_step_n_policy, FS_KERNEL_PACKED = fs_step_n_packed.  For naming profiles and roofline lines; NULL for a bad handle or flags.
 * The string stays valid until the calling thread's next call. */
#define FS_KERNEL_HASHED 1
#define FS_KERNEL_POLICY 2
#define FS_KERNEL_PACKED 4  /* fs_step_n_packed */
/* fs_step_skip_policy (alone; n_steps = decisions): NULL on a handle the call refuses.  (8 is not a flag.) */
#define FS_KERNEL_SKIP_POLICY 16
/* fs_step_n_selfplay (alone; "fsk::selfplay::k_step_n_selfplay<0>"): NULL on a handle the call refuses */
#define FS_KERNEL_SELFPLAY 32
/* fs_step_skip_selfplay (alone; n_steps = decisions; "fsk::selfplay::k_step_skip_selfplay<0>"): NULL on a
 * handle the call refuses */
#define FS_KERNEL_SKIP_SELFPLAY 64
/* fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool (each alone; "fsk::selfplay::k_step_n_selfplay_pool<0>",
 * "fsk::selfplay::k_step_skip_pool_selfplay<0>"): NULL on a handle the call refuses */
#define FS_KERNEL_SELFPLAY_POOL 128
#define FS_KERNEL_SKIP_SELFPLAY_POOL 256
/* fs_step_n_league / fs_step_skip_league (each alone; "fsk::league::k_step_n_league<0>",
 * "fsk::league::k_step_skip_league<0>"): NULL on a handle the call refuses, a mixed group included */
#define FS_KERNEL_LEAGUE 512
#define FS_KERNEL_SKIP_LEAGUE 1024
const char* fs_step_kernel(fs_handle h, int n_steps, int flags);
void fs_destroy(fs_handle h);
/* Last error message of h (or of the last failed fs_create when h is NULL). */
const char* fs_last_error(fs_handle h);

#ifdef __cplusplus
}
#endif
#endif /* FOOTSIES_H */
