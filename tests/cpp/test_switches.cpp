// CPU-side unit test of the developer switches (yocto-hair_amd/host/switches.h): every accessor against the environment, set and unset
// between calls: compiled and run by tests/test_abi.py::test_developer_switches (g++ only, no HIP, no GPU).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "switches.h"

static int fails = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      fails++;                                                   \
    }                                                            \
  } while (0)

// the accessor's value with the variable set to `value` (NULL: unset); the variable is left unset
template <class F>
static auto with(const char* name, const char* value, F&& accessor) {
  value ? setenv(name, value, 1) : unsetenv(name);
  auto r = accessor();
  unsetenv(name);
  return r;
}

int main() {
  using namespace yhh;
  {  // the switches that are on when SET, whatever their text
    struct { const char* name; bool (*on)(); } set_is_on[] = {{"YHAIR_NO_TRIALS", no_trials}, {"YHAIR_NO_TRIAL_CACHE", no_trial_cache},
        {"YHAIR_NO_DISK_CACHE", no_disk_cache}, {"YHAIR_NO_PROBE", no_probe}, {"YHAIR_ST_WAVELOG", st_wavelog}};
    for (auto& s : set_is_on) {
      CHECK(!with(s.name, nullptr, s.on));
      CHECK(with(s.name, "0", s.on));
      CHECK(with(s.name, "1", s.on));
      CHECK(with(s.name, "yes", s.on));
    }
  }
  {  // ... and those that are on when set to a non-zero number: YHAIR_TIMING=0 is off
    CHECK(!with("YHAIR_TIMING", nullptr, timing));
    CHECK(!with("YHAIR_TIMING", "0", timing));
    CHECK(with("YHAIR_TIMING", "1", timing));
    CHECK(!with("YHAIR_TIMING", "yes", timing));
    CHECK(with("YHAIR_ST_PROF", nullptr, st_prof) == 0);
    CHECK(with("YHAIR_ST_PROF", "0", st_prof) == 0);
    CHECK(with("YHAIR_ST_PROF", "1", st_prof) == 1);
    CHECK(with("YHAIR_ST_PROF", "2", st_prof) == 2);
    CHECK(with("YHAIR_ST_PROF", "3", st_prof) == 1);
    CHECK(with("YHAIR_ST_PROF", "yes", st_prof) == 0);
  }
  {  // YHAIR_SHAPE: clamped to the table of launch shapes, -1 when unset
    CHECK(with("YHAIR_SHAPE", nullptr, forced_shape) == -1);
    CHECK(with("YHAIR_SHAPE", "-3", forced_shape) == 0);
    CHECK(with("YHAIR_SHAPE", "0", forced_shape) == 0);
    char last[16];
    snprintf(last, sizeof(last), "%d", YH_SHAPES - 1);
    CHECK(with("YHAIR_SHAPE", last, forced_shape) == YH_SHAPES - 1);
    CHECK(with("YHAIR_SHAPE", "99", forced_shape) == YH_SHAPES - 1);
  }
  {  // YHAIR_ST_SLOTS: a multiple of 64 in [64, 4096], 0 when unset; YHAIR_ST_WAVES: waves per CU as an occupancy in workgroups
    CHECK(with("YHAIR_ST_SLOTS", nullptr, st_slots) == 0);
    CHECK(with("YHAIR_ST_SLOTS", "1", st_slots) == 64);
    CHECK(with("YHAIR_ST_SLOTS", "100", st_slots) == 64);
    CHECK(with("YHAIR_ST_SLOTS", "4096", st_slots) == 4096);
    CHECK(with("YHAIR_ST_SLOTS", "100000", st_slots) == 4096);
    auto occupancy = [] { return st_occupancy(4, 4); };  // four workgroups of four waves fit
    CHECK(with("YHAIR_ST_WAVES", nullptr, occupancy) == 4);
    CHECK(with("YHAIR_ST_WAVES", "0", occupancy) == 1);
    CHECK(with("YHAIR_ST_WAVES", "5", occupancy) == 2);
    CHECK(with("YHAIR_ST_WAVES", "8", occupancy) == 2);
    CHECK(with("YHAIR_ST_WAVES", "64", occupancy) == 4);
  }
  {  // YHAIR_INTERSECT: quad, or the lane kernel at 4 .. 8 waves per SIMD; anything else leaves the choice to the batch
    auto is = [](const char* value, int mode, int waves) {
      return with("YHAIR_INTERSECT", value, [&] {  // (text points into the environment: compared while the variable is set)
        const IntersectSwitch s = intersect_switch();
        return s.mode == mode && s.waves == waves && (value ? s.text && !strcmp(s.text, value) : !s.text);
      });
    };
    CHECK(is(nullptr, IntersectSwitch::AUTO, 5));
    CHECK(is("quad", IntersectSwitch::QUAD, 5));
    CHECK(is("lane3", IntersectSwitch::LANES, 4));
    CHECK(is("lane5", IntersectSwitch::LANES, 5));
    CHECK(is("lane9", IntersectSwitch::LANES, 8));
    CHECK(is("bogus", IntersectSwitch::AUTO, 5));
  }
  {  // YHAIR_BVH, YHAIR_GATHER: their two words, anything else is the default
    CHECK(with("YHAIR_BVH", nullptr, bvh_switch) == BVH_BY_SIZE && with("YHAIR_BVH", "gpu", bvh_switch) == BVH_BY_SIZE);
    CHECK(with("YHAIR_BVH", "host", bvh_switch) == BVH_HOST && with("YHAIR_BVH", "device", bvh_switch) == BVH_DEVICE);
    CHECK(with("YHAIR_GATHER", nullptr, gather_switch) == GATHER_BY_DEVICES && with("YHAIR_GATHER", "ring", gather_switch) == GATHER_BY_DEVICES);
    CHECK(with("YHAIR_GATHER", "rccl", gather_switch) == GATHER_RCCL && with("YHAIR_GATHER", "peer", gather_switch) == GATHER_PEER);
  }
  {  // YHAIR_DEVICE_SHARE: the number (one at least) and the text the key of the trial record on disk holds ("1" when unset, else verbatim)
    auto key_is = [](const char* value, const char* key) { return !strcmp(with("YHAIR_DEVICE_SHARE", value, [] { return std::string(device_share_key()); }).c_str(), key); };
    CHECK(with("YHAIR_DEVICE_SHARE", nullptr, device_share) == 1 && key_is(nullptr, "1"));
    CHECK(with("YHAIR_DEVICE_SHARE", "0", device_share) == 1 && key_is("0", "0"));
    CHECK(with("YHAIR_DEVICE_SHARE", "4", device_share) == 4 && key_is("4", "4"));
  }
  {  // YHAIR_CACHE_DIR: verbatim, NULL when unset
    CHECK(with("YHAIR_CACHE_DIR", nullptr, cache_dir) == nullptr);
    CHECK(with("YHAIR_CACHE_DIR", "/tmp/x", [] { return std::string(cache_dir()); }) == "/tmp/x");
  }
  {  // YHAIR_LAUNCH_TIMEOUT_S: a positive number of seconds, clamped to what the wait's nanosecond clock can hold, else the default
    CHECK(with("YHAIR_LAUNCH_TIMEOUT_S", nullptr, launch_timeout_s) == 1800.0);
    CHECK(with("YHAIR_LAUNCH_TIMEOUT_S", "0.25", launch_timeout_s) == 0.25);
    CHECK(with("YHAIR_LAUNCH_TIMEOUT_S", "-3", launch_timeout_s) == 1800.0);
    CHECK(with("YHAIR_LAUNCH_TIMEOUT_S", "soon", launch_timeout_s) == 1800.0);
    CHECK(with("YHAIR_LAUNCH_TIMEOUT_S", "1e12", launch_timeout_s) == 1e8);
    CHECK(with("YHAIR_LAUNCH_TIMEOUT_S", "inf", launch_timeout_s) == 1e8);
  }
  {  // nothing is frozen at first use: a value changed between two calls is seen by the second
    setenv("YHAIR_ST_PROF", "1", 1), setenv("YHAIR_NO_TRIALS", "1", 1), setenv("YHAIR_DEVICE_SHARE", "2", 1), setenv("YHAIR_SHAPE", "3", 1), setenv("YHAIR_TIMING", "1", 1);
    CHECK(st_prof() == 1 && no_trials() && device_share() == 2 && forced_shape() == 3 && timing());
    setenv("YHAIR_ST_PROF", "2", 1), unsetenv("YHAIR_NO_TRIALS"), setenv("YHAIR_DEVICE_SHARE", "8", 1), setenv("YHAIR_SHAPE", "4", 1), setenv("YHAIR_TIMING", "0", 1);
    CHECK(st_prof() == 2 && !no_trials() && device_share() == 8 && forced_shape() == 4 && !timing());
    unsetenv("YHAIR_ST_PROF"), unsetenv("YHAIR_DEVICE_SHARE"), unsetenv("YHAIR_SHAPE"), unsetenv("YHAIR_TIMING");
    CHECK(st_prof() == 0 && device_share() == 1 && forced_shape() == -1 && !timing());
  }
  printf(fails ? "switches: %d checks FAILED\n" : "switches: all checks passed\n", fails);
  return fails ? 1 : 0;
}
