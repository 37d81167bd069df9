// env_case.cpp -- the accessors of sparse_matrix_math_amd/csrc/smm_env.h on their own: host compiler, AddressSanitizer + UBSan, no library.
// A ONCE switch can be asked for the first time only once per process, so every ONCE check below uses a switch of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sparse_matrix_math_amd/csrc/smm_env.h"

namespace env = smm::env;

static int failed = 0;
#define CHECK(cond)                                                     \
	do {                                                                \
		if (!(cond)) {                                                  \
			std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
			++failed;                                                   \
		}                                                               \
	} while (0)

static void put(env::Id id, const char* text) {
	if (text) {
		setenv(env::TABLE[id].name, text, 1);
	} else {
		unsetenv(env::TABLE[id].name);
	}
}

int main() {
	for (int i = 0; i < env::COUNT; ++i) unsetenv(env::TABLE[i].name);
	static_assert(env::TABLE[env::TILE_BATCH].policy == env::EACH && env::TABLE[env::SWEEP_WAVES_PER_LEVEL].policy == env::EACH &&
	                  env::TABLE[env::RCCL_PATH].policy == env::EACH && env::TABLE[env::P2P].policy == env::EACH,
	              "the EACH switches this program uses");
	static_assert(env::TABLE[env::PATTERN_WAVE].policy == env::ONCE && env::TABLE[env::NT_OUT].policy == env::ONCE &&
	                  env::TABLE[env::MARCH_MIN_ROWS].policy == env::ONCE && env::TABLE[env::COMM_TIMEOUT_S].policy == env::ONCE &&
	                  env::TABLE[env::MARCH_R].policy == env::ONCE && env::TABLE[env::TRACE_SETUP].policy == env::ONCE,
	              "the ONCE switches this program uses");

	// ---- EACH: every ask looks the variable up
	CHECK(env::intOr(env::TILE_BATCH, -3) == -3);  // unset: the caller's default
	CHECK(env::raw(env::TILE_BATCH) == nullptr && !env::isSet(env::TILE_BATCH));
	put(env::TILE_BATCH, "7");
	CHECK(env::intOr(env::TILE_BATCH, -3) == 7);
	put(env::TILE_BATCH, "");
	CHECK(env::intOr(env::TILE_BATCH, -3) == 0 && env::isSet(env::TILE_BATCH));  // atoi(""): 0, not the default
	put(env::TILE_BATCH, "abc");
	CHECK(env::intOr(env::TILE_BATCH, -3) == 0);
	put(env::TILE_BATCH, "13");  // a change between two asks is followed
	CHECK(env::intOr(env::TILE_BATCH, -3) == 13);
	put(env::TILE_BATCH, nullptr);
	CHECK(env::intOr(env::TILE_BATCH, -3) == -3);

	CHECK(env::flagOr(env::P2P, true) && !env::flagOr(env::P2P, false));
	put(env::P2P, "0");
	CHECK(!env::flagOr(env::P2P, true));
	put(env::P2P, "2");
	CHECK(env::flagOr(env::P2P, false));
	put(env::P2P, "abc");
	CHECK(!env::flagOr(env::P2P, true));

	CHECK(env::longOr(env::TILE_BATCH, 1LL << 40) == 1LL << 40);
	put(env::TILE_BATCH, "17179869184");
	CHECK(env::longOr(env::TILE_BATCH, -1) == 17179869184LL);
	CHECK(env::doubleOr(env::SWEEP_WAVES_PER_LEVEL, 4.0) == 4.0);
	put(env::SWEEP_WAVES_PER_LEVEL, "0.25");
	CHECK(env::doubleOr(env::SWEEP_WAVES_PER_LEVEL, 4.0) == 0.25);
	put(env::SWEEP_WAVES_PER_LEVEL, "");
	CHECK(env::doubleOr(env::SWEEP_WAVES_PER_LEVEL, 4.0) == 0.0);

	CHECK(env::raw(env::RCCL_PATH) == nullptr);
	put(env::RCCL_PATH, "/somewhere/librccl.so.1");
	CHECK(env::raw(env::RCCL_PATH) && std::strcmp(env::raw(env::RCCL_PATH), "/somewhere/librccl.so.1") == 0);
	put(env::RCCL_PATH, nullptr);
	CHECK(env::raw(env::RCCL_PATH) == nullptr);

	// ---- ONCE: the first ask decides, whatever the type asked for later
	put(env::PATTERN_WAVE, "7");
	CHECK(env::intOr(env::PATTERN_WAVE, -1) == 7);
	put(env::PATTERN_WAVE, "9");
	CHECK(env::intOr(env::PATTERN_WAVE, -1) == 7);
	put(env::PATTERN_WAVE, nullptr);
	CHECK(env::intOr(env::PATTERN_WAVE, -1) == 7 && env::isSet(env::PATTERN_WAVE) && env::flagOr(env::PATTERN_WAVE, false));
	CHECK(env::raw(env::PATTERN_WAVE) && std::strcmp(env::raw(env::PATTERN_WAVE), "7") == 0);  // (a copy: the variable is gone)

	CHECK(env::intOr(env::NT_OUT, -1) == -1);  // unset at the first ask: the default for good
	put(env::NT_OUT, "1");
	CHECK(env::intOr(env::NT_OUT, -1) == -1 && env::intOr(env::NT_OUT, 5) == 5 && !env::isSet(env::NT_OUT) && env::raw(env::NT_OUT) == nullptr);

	put(env::MARCH_MIN_ROWS, "17179869184");
	CHECK(env::longOr(env::MARCH_MIN_ROWS, -1) == 17179869184LL);
	put(env::MARCH_MIN_ROWS, "5");
	CHECK(env::longOr(env::MARCH_MIN_ROWS, -1) == 17179869184LL);
	put(env::COMM_TIMEOUT_S, "0.25");
	CHECK(env::doubleOr(env::COMM_TIMEOUT_S, 180.0) == 0.25);
	put(env::COMM_TIMEOUT_S, nullptr);
	CHECK(env::doubleOr(env::COMM_TIMEOUT_S, 180.0) == 0.25);

	put(env::MARCH_R, "abc");  // first asked for its presence, then for its value: one latch
	CHECK(env::isSet(env::MARCH_R));
	put(env::MARCH_R, "8");
	CHECK(env::intOr(env::MARCH_R, 4) == 0);
	put(env::TRACE_SETUP, "");
	CHECK(!env::flagOr(env::TRACE_SETUP, true) && env::isSet(env::TRACE_SETUP));

	std::printf("env_case: %d switches, %d failed\n", static_cast<int>(env::COUNT), failed);
	return failed ? 1 : 0;
}
