// CPU-side check of the text the developer reports of a k_stream launch print (yocto-hair_amd/host/stream_report.cpp — the REAL file, compiled
// into this test with the device's copy mocked): tools/ read these lines. Two wave logs of eight waves (the second prints the correlation
// with the first) and one table of the instrumented build's 64 counters go to stderr; tests/test_abi.py::test_stream_report_text compares it
// with tests/golden/stream_report.txt, which the code BEFORE the reports moved out of stream_impl printed for these inputs.
#include "../../yocto-hair_amd/host/stream_report.cpp"

extern "C" {
hipError_t  hipFree(void*) { return hipSuccess; }
hipError_t  hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind) { memcpy(dst, src, n); return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "mock"; }
}
int fail(yh_context*, int code, const char*, ...) { return code; }

int main() {
  yh_context ctx{};
  ctx.num_cus = 2;  // two workgroups per dispatch round: four workgroups of two waves are rounds 0 and 1
  // {begin, end} per wave, in the device's 100 MHz ticks
  const unsigned long long first[16]  = {1000, 901000, 1200, 650000, 1100, 1501000, 1300, 1250000, 400000, 1400000, 400500, 1100000, 420000, 1480000, 430000, 990000};
  const unsigned long long second[16] = {5000, 880000, 5100, 700000, 5300, 1450000, 5200, 1300000, 390000, 1405000, 391000, 1000000, 410000, 1505000, 415000, 1010000};
  report_stream_waves(&ctx, first, 8, 2);
  report_stream_waves(&ctx, second, 8, 2);
  unsigned long long c[64];
  for (int k = 0; k < 64; k++) c[k] = 1000ull * (unsigned long long)(k + 1) + (unsigned long long)((k * 37) % 11);
  c[9] = 0, c[40] = 0;  // a stage without trips and a branch that never ran: their means print as 0.0
  ctx.d_st_prof.p = c, ctx.last_ms = 12.5f;
  const int rc = report_stream_prof(&ctx, 4, 2, 128);
  ctx.d_st_prof.p = nullptr;
  return rc;
}
