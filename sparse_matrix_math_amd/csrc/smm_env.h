// smm_env.h -- every environment variable libsmm_hip.so reads: one table, and the only getenv of the library.
// Standard library only (no HIP): a plain host compiler takes this header on its own (tests/cpp/env_case.cpp).
// INTEGRATION.md, "Environment switches", lists the same rows with their defaults; tests/test_env_switches_cpu.py keeps the two alike.
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>

namespace smm {
namespace env {

// ONCE: latched at the first ask for that switch in the process (not at library load: callers may set it after loading the library);
// EACH: looked up at every ask -- a property of the handle being created or of the call, which tests and bench.py change in-process
enum Policy { ONCE, EACH };
// SPEED: same bits, only time; ARITH: another kernel, tile shape or grid -- the grouping of a row's sum or of the dot products fused into
// an SpMV may change, or a preconditioner becomes another operator; TRANSPORT: devices, multi-GPU data movement and its time limits;
// DIAG: prints; LAB: hooks of tests and lab scripts that production code never sets
enum Effect { SPEED, ARITH, TRANSPORT, DIAG, LAB };

// X(identifier, variable, policy, effect, what it does)
#define SMM_ENV_SWITCHES(X)                                                                                                                  \
	X(AUTO_DICT, "SMM_HIP_AUTO_DICT", ONCE, ARITH, "0: the automatic PATTERN attempt stops at the row masks and never takes the dictionary (CODES) encoding") \
	X(AUTO_PATTERN, "SMM_HIP_AUTO_PATTERN", ONCE, ARITH, "0: AUTO and the solvers never adopt the PATTERN family, the matrix stays on STREAM") \
	X(AUTO_PATTERN_MIN_NNZ, "SMM_HIP_AUTO_PATTERN_MIN_NNZ", ONCE, ARITH, "stored entries from which a single SpMV tries the PATTERN family") \
	X(BICGSTAB_RESIDENT, "SMM_HIP_BICGSTAB_RESIDENT", ONCE, ARITH, "initial mode of the single-launch BiCGStab: 0 off, 1 auto, 2 require (smm_hip_bicgstab_resident changes it)") \
	X(BLOCK_BRICKS, "SMM_HIP_BLOCK_BRICKS", ONCE, ARITH, "0: block preconditioners always cut contiguous blocks, never grid bricks") \
	X(BLOCK_DEPTH, "SMM_HIP_BLOCK_DEPTH", ONCE, SPEED, "1 / 2 / 4 / 8: chunks in flight per sweep of the block apply kernel, where compiled") \
	X(BLOCK_FUSE_SPMV, "SMM_HIP_BLOCK_FUSE_SPMV", EACH, ARITH, "0 / 1 (first character): never / always run the solver's SpMV inside the block apply launch") \
	X(BLOCK_KREG, "SMM_HIP_BLOCK_KREG", EACH, LAB, "2 / 3 / 4 / 8: at least that many register entries per row of a block preconditioner; -8: force its overflow path (tests)") \
	X(BLOCK_LEVEL_CAP, "SMM_HIP_BLOCK_LEVEL_CAP", EACH, ARITH, "default level cut of a block preconditioner (below 2: none; at most 4095)") \
	X(BLOCK_ROWS, "SMM_HIP_BLOCK_ROWS", EACH, ARITH, "default rows per block of a block preconditioner (clamped to the supported range)") \
	X(CG_FUSE_P, "SMM_HIP_CG_FUSE_P", ONCE, SPEED, "0: ConjugateGradient never forms its next direction inside the SpMV launch") \
	X(CG_LAZY_X, "SMM_HIP_CG_LAZY_X", ONCE, SPEED, "0: ConjugateGradient never defers its x update") \
	X(CG_RESIDENT, "SMM_HIP_CG_RESIDENT", ONCE, ARITH, "initial mode of the single-launch ConjugateGradient: 0 off, 1 auto, 2 require (smm_hip_cg_resident changes it)") \
	X(COMM_TIMEOUT_S, "SMM_HIP_COMM_TIMEOUT_S", ONCE, TRANSPORT, "seconds a distributed call waits on a stream that may carry RCCL work before it aborts the communicator") \
	X(CONST_MARCH, "SMM_HIP_CONST_MARCH", ONCE, ARITH, "0: constant-diagonal matrices keep the gather kernel, never the 2.5-D march kernels") \
	X(CONST_WGS_PER_CU, "SMM_HIP_CONST_WGS_PER_CU", ONCE, ARITH, "workgroups per CU of the constant-diagonal gather kernel (at least 1)") \
	X(DEVICE, "SMM_HIP_DEVICE", EACH, TRANSPORT, "the device a process that never calls smm_hip_init gets at its first call") \
	X(DIST_DEBUG, "SMM_HIP_DIST_DEBUG", EACH, DIAG, "set (any value): every distributed CG solve prints what its loop chose on stderr") \
	X(FULL_ROWS, "SMM_HIP_FULL_ROWS", ONCE, ARITH, "0: the PATTERN tile kernel takes its general path for every row; the slots kernel is off") \
	X(HALO_CHUNKS, "SMM_HIP_HALO_CHUNKS", EACH, TRANSPORT, "2 .. 4: the halo travels in that many pieces (implies the collectives); the ranks agree on the smallest request") \
	X(HALO_FIRST, "SMM_HIP_HALO_FIRST", ONCE, TRANSPORT, "0: update kernels do not write the rows other ranks need first; same bits") \
	X(LAB_SELF_P2P, "SMM_HIP_LAB_SELF_P2P", EACH, LAB, "1, single-rank communicator only: set the peer-to-peer slots up with one rank") \
	X(LAB_SELF_SPLIT, "SMM_HIP_LAB_SELF_SPLIT", EACH, LAB, "single-rank communicator only: columns beyond this window count as remote, as on a rank of a many-GPU run") \
	X(MARCH_FUSE_FULL_TILES, "SMM_HIP_MARCH_FUSE_FULL_TILES", ONCE, ARITH, "1: ConjugateGradient's launches on the march kernel keep full tiles") \
	X(MARCH_MIN_ROWS, "SMM_HIP_MARCH_MIN_ROWS", ONCE, ARITH, "rows from which the march kernels serve a matrix, all four thresholds (smm_hip_set_march_min_rows wins)") \
	X(MARCH_R, "SMM_HIP_MARCH_R", ONCE, ARITH, "4 / 8: rows per lane of the constant-diagonal march kernel; set to anything: no half tiles, no fused direction") \
	X(MARCH_WGS_PER_CU, "SMM_HIP_MARCH_WGS_PER_CU", ONCE, ARITH, "workgroups per CU of the march kernels") \
	X(MARCH_ZC, "SMM_HIP_MARCH_ZC", ONCE, ARITH, "planes per unit of the march kernels") \
	X(MASKS_MARCH, "SMM_HIP_MASKS_MARCH", ONCE, ARITH, "0: row-mask matrices with values read keep the wave kernel, never the march form") \
	X(MASKS_MARCH_Q, "SMM_HIP_MASKS_MARCH_Q", ONCE, ARITH, "2 / 4: sub-steps per tile of the masks march kernel") \
	X(NT_OUT, "SMM_HIP_NT_OUT", ONCE, ARITH, "0 / 1: never / always store SpMV outputs non-temporally; also moves what follows that policy (half tiles, fused direction)") \
	X(P2P, "SMM_HIP_P2P", EACH, TRANSPORT, "0 on any rank: every rank keeps the communicator's collectives") \
	X(P2P_DIRECT_SHARE, "SMM_HIP_P2P_DIRECT_SHARE", EACH, TRANSPORT, "share of a halo segment sent over the direct link (0.05 .. 1)") \
	X(P2P_HALO, "SMM_HIP_P2P_HALO", EACH, TRANSPORT, "0: the hybrid -- halo by grouped send / receive, scalars through the peer-to-peer slots") \
	X(P2P_RELAYS, "SMM_HIP_P2P_RELAYS", EACH, TRANSPORT, "relay ranks per halo segment of the peer-to-peer transport") \
	X(P2P_TIMEOUT_S, "SMM_HIP_P2P_TIMEOUT_S", ONCE, TRANSPORT, "seconds a peer-to-peer wait may take before the call fails with SMM_HIP_ERR_COMM") \
	X(PATTERN_CONST, "SMM_HIP_PATTERN_CONST", ONCE, SPEED, "0: the PATTERN analysis does not look for constant diagonals; values[] is always read") \
	X(PATTERN_SLOTS, "SMM_HIP_PATTERN_SLOTS", ONCE, SPEED, "0: never the slots kernel; 3: wherever it applies, walked by the sweep kernel; other: wherever it applies (a handle's own mode wins)") \
	X(PATTERN_SWEEP_ROWS, "SMM_HIP_PATTERN_SWEEP_ROWS", ONCE, SPEED, "8 / 16 / 32: 64-row waves a hardware wave of the sweep kernel holds open (smm_hip_set_pattern_sweep_rows wins)") \
	X(PATTERN_SWEEP_WGS, "SMM_HIP_PATTERN_SWEEP_WGS", ONCE, SPEED, "1 .. 8: workgroups per CU of the sweep kernel") \
	X(PATTERN_VARIANT, "SMM_HIP_PATTERN_VARIANT", ONCE, ARITH, "0: the pipelined row-per-lane PATTERN kernel for every lane count; tile and slots kernels are off") \
	X(PATTERN_WAVE, "SMM_HIP_PATTERN_WAVE", ONCE, ARITH, "workgroups per CU of the wave-private PATTERN kernel; 0: off, the tile kernels serve those matrices") \
	X(PRELOAD, "SMM_HIP_PRELOAD", ONCE, SPEED, "0: smm_hip_init does not load the hot path's code objects ahead of the first call") \
	X(RCCL_PATH, "SMM_HIP_RCCL_PATH", EACH, TRANSPORT, "librccl to dlopen when the process has none mapped, tried before the standard names") \
	X(RESIDENT_LAB, "SMM_RESIDENT_LAB", EACH, LAB, "builds with -DSMM_RESIDENT_LAB only: lab bits of the single-launch CG (2: unbounded barrier waits)") \
	X(SOLVER_PATTERN_MIN_NNZ, "SMM_HIP_SOLVER_PATTERN_MIN_NNZ", ONCE, ARITH, "stored entries from which a solver tries the PATTERN family before its loop") \
	X(SPLIT_SPMV, "SMM_HIP_SPLIT_SPMV", EACH, TRANSPORT, "0: a rank's SpMV stays two launches; 2: one launch also between ranks that share a GPU; same SpMV bits") \
	X(SPLIT_SUMS_LDS, "SMM_HIP_SPLIT_SUMS_LDS", EACH, TRANSPORT, "bytes of LDS the row sums of the one-launch SpMV may take (0: always through out[])") \
	X(SPMV_FAMILY, "SMM_HIP_SPMV_FAMILY", EACH, ARITH, "kernel family a new matrix starts with (the VECTOR or STREAM value of smm_hip.h)") \
	X(SPMV_LANES, "SMM_HIP_SPMV_LANES", EACH, ARITH, "lanes per row a new matrix starts with (a power of two, 1 .. 64)") \
	X(STAGED_COPIES, "SMM_HIP_STAGED_COPIES", ONCE, SPEED, "0: host-pointer entry points hand the caller's arrays to hipMemcpyAsync directly") \
	X(STREAM_NV, "SMM_HIP_STREAM_NV", EACH, ARITH, "LDS capacity of a STREAM tile, in staging pieces") \
	X(STREAM_VARIANT, "SMM_HIP_STREAM_VARIANT", ONCE, ARITH, "0 / 1: the pipelined / the TILE kernel of the STREAM family wherever it exists") \
	X(STREAM_WGS_PER_CU, "SMM_HIP_STREAM_WGS_PER_CU", ONCE, ARITH, "workgroups per CU of the persistent STREAM / PATTERN grids (at least 1)") \
	X(SWEEP, "SMM_HIP_SWEEP", EACH, SPEED, "what AUTO means for the triangular sweeps: an SMM_SWEEP_* value of smm_hip.h") \
	X(SWEEP_WAVES, "SMM_HIP_SWEEP_WAVES", EACH, SPEED, "wavefronts of a synchronisation-free sweep launch") \
	X(SWEEP_WAVES_PER_LEVEL, "SMM_HIP_SWEEP_WAVES_PER_LEVEL", EACH, SPEED, "levels' worth of rows a synchronisation-free sweep launch is sized to (at least 0.25)") \
	X(THIN_REMOTE, "SMM_HIP_THIN_REMOTE", EACH, TRANSPORT, "0: the remote half of a rank's SpMV passes over all rows; same bits") \
	X(TILE_BATCH, "SMM_HIP_TILE_BATCH", EACH, ARITH, "gathers per batch of the TILE kernels (STREAM: 4 .. 16; PATTERN: 8, 13 or 16)") \
	X(TRACE_SETUP, "SMM_HIP_TRACE_SETUP", ONCE, DIAG, "1: the host-side stages of one-off set-up work print their wall time on stderr") \
	X(UPDATE_NT, "SMM_HIP_UPDATE_NT", ONCE, SPEED, "0 / 1: never / always use non-temporal loads and stores in the solvers' update kernels") \
	X(XCD_CHUNK_TILES, "SMM_HIP_XCD_CHUNK_TILES", EACH, ARITH, "tiles dealt to one XCD in turn (0: one contiguous eighth each)") \
	X(ZERO_START, "SMM_HIP_ZERO_START", EACH, SPEED, "0: BiCGStab, ConjugateGradient and ConjugateGradientSquared launch the set-up SpMV r = b - A x0 also from an all-zero x0")

enum Id {
#define SMM_ENV_ID(id, name, policy, effect, what) id,
	SMM_ENV_SWITCHES(SMM_ENV_ID)
#undef SMM_ENV_ID
	COUNT
};

struct Row {
	const char* name;
	Policy policy;
	Effect effect;
	const char* what;
};
inline constexpr Row TABLE[COUNT] = {
#define SMM_ENV_ROW(id, name, policy, effect, what) {name, policy, effect, what},
	SMM_ENV_SWITCHES(SMM_ENV_ROW)
#undef SMM_ENV_ROW
};

// what a ONCE switch held at its first ask, parsed every way there: later asks are loads (text == nullptr: it was unset)
struct Latched {
	const char* text;
	int i;
	long long ll;
	double d;
};
inline std::atomic<const Latched*> g_latched[COUNT];

inline const Latched* latched(Id id) {
	const Latched* seen = g_latched[id].load(std::memory_order_acquire);
	if (seen) return seen;
	Latched* mine = new Latched{nullptr, 0, 0, 0.0};
	if (const char* e = std::getenv(TABLE[id].name)) {  // (a copy: the environment's own string may go away)
		mine->text = std::strcpy(new char[std::strlen(e) + 1], e);
		mine->i = std::atoi(e);
		mine->ll = std::atoll(e);
		mine->d = std::atof(e);
	}
	if (g_latched[id].compare_exchange_strong(seen, mine, std::memory_order_acq_rel, std::memory_order_acquire)) return mine;  // (kept for the process)
	delete[] mine->text;  // another thread latched first: its answer holds
	delete mine;
	return seen;
}

// the variable's text, or nullptr when it is unset
inline const char* raw(Id id) { return TABLE[id].policy == EACH ? std::getenv(TABLE[id].name) : latched(id)->text; }
inline bool isSet(Id id) { return raw(id) != nullptr; }

// unset: `unset`; else atoi / atoll / atof of the text (so "" and "abc" give 0, not `unset`)
inline int intOr(Id id, int unset) {
	if (TABLE[id].policy == ONCE) return latched(id)->text ? latched(id)->i : unset;
	const char* e = std::getenv(TABLE[id].name);
	return e ? std::atoi(e) : unset;
}
inline long long longOr(Id id, long long unset) {
	if (TABLE[id].policy == ONCE) return latched(id)->text ? latched(id)->ll : unset;
	const char* e = std::getenv(TABLE[id].name);
	return e ? std::atoll(e) : unset;
}
inline double doubleOr(Id id, double unset) {
	if (TABLE[id].policy == ONCE) return latched(id)->text ? latched(id)->d : unset;
	const char* e = std::getenv(TABLE[id].name);
	return e ? std::atof(e) : unset;
}
inline bool flagOr(Id id, bool unset) { return intOr(id, unset ? 1 : 0) != 0; }

}  // namespace env
}  // namespace smm
