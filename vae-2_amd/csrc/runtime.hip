// Runtime glue of libvae2_hip.so: the kernel launch log behind VAE2_LAUNCH, the per-thread
// last error behind VAE2_REQUIRE / check_launch, and the ABI version.
#include "common.h"

#include <cxxabi.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace vae2 {

// ------------------------------------------------------ launch log ----
static std::atomic<bool> g_klog{false};
static thread_local std::vector<const void*> g_klog_v;

void note_kernel(const void* host_fn) {
  if (g_klog.load(std::memory_order_relaxed)) g_klog_v.push_back(host_fn);
}

// "void vae2::dconv3_kernel<4, 2, false>(vae2::DConv)" -> "dconv3_kernel<4, 2, false>"
static std::string kernel_label(const void* fn) {
  const char* raw = hipKernelNameRefByPtr(fn, nullptr);
  if (!raw) return "?";
  int st = 0;
  char* dem = abi::__cxa_demangle(raw, nullptr, nullptr, &st);
  std::string s = (st == 0 && dem) ? dem : raw;
  std::free(dem);
  if (s.rfind("void ", 0) == 0) s = s.substr(5);
  int depth = 0;
  for (size_t i = 0; i < s.size(); ++i) {  // drop the parameter list
    if (s[i] == '<') ++depth;
    if (s[i] == '>') --depth;
    if (s[i] == '(' && depth == 0) { s = s.substr(0, i); break; }
  }
  size_t pos;
  while ((pos = s.find("vae2::")) != std::string::npos) s.erase(pos, 6);
  return s;
}

// ------------------------------------------------------------- errors ----
static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(const char* fn, const std::string& msg) {
  set_error(std::string(fn) + ": " + msg);
  return -22;
}

int check_launch(const char* fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(fn) + ": " + hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace vae2

using namespace vae2;

extern "C" {

int vae2_abi_version(void) { return VAE2_ABI_VERSION; }

const char* vae2_last_error(void) { return g_last_error.c_str(); }

int vae2_kernel_log(int enable) {
  g_klog.store(enable != 0);
  g_klog_v.clear();
  return 0;
}

int64_t vae2_kernel_log_read(char* buf, int64_t len) {
  std::string out;
  for (size_t i = 0; i < g_klog_v.size(); ++i) {
    if (i) out += ';';
    out += kernel_label(g_klog_v[i]);
  }
  const int64_t n = (int64_t)g_klog_v.size();
  g_klog_v.clear();
  if (buf && len > 0) {
    const size_t m = out.size() < (size_t)(len - 1) ? out.size() : (size_t)(len - 1);
    std::memcpy(buf, out.data(), m);
    buf[m] = 0;
  }
  return n;
}

}  // extern "C"
