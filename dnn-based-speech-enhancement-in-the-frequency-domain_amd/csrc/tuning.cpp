// The process-wide tuning table (tuning.h).
#include "tuning.h"

#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

namespace sefd {
namespace {
std::mutex g_mu;
std::map<std::string, std::unique_ptr<std::string>, std::less<>> g_tab;   // values behind stable pointers: tune_str hands out c_str(); less<>: lookup by string_view, no allocation
std::vector<std::unique_ptr<std::string>> g_retired;           // replaced values stay alive (a caller may still hold the old pointer)
std::vector<std::pair<std::string, std::string>> g_env;        // the pairs of SEFD_TUNING: what tune_clear() returns to
bool g_init = false;

void seed_locked() {
  for (const auto& kv : g_env) g_tab[kv.first] = std::make_unique<std::string>(kv.second);
}

void init_locked() {
  if (g_init) return;
  g_init = true;
  const char* e = std::getenv("SEFD_TUNING");                  // the ONE environment variable of the library, parsed once
  if (!e) return;
  std::string s(e);
  size_t i = 0;
  while (i < s.size()) {
    size_t j = s.find_first_of(",; ", i);
    if (j == std::string::npos) j = s.size();
    const std::string kv = s.substr(i, j - i);
    const size_t eq = kv.find('=');
    if (eq != std::string::npos && eq > 0) g_env.emplace_back(kv.substr(0, eq), kv.substr(eq + 1));
    i = j + 1;
  }
  seed_locked();
}

// the one parser: every typed read goes through here, under the lock (the value's text may be retired by a concurrent tune_set)
template <typename F>
auto with_value(const char* knob, F f) {
  std::lock_guard<std::mutex> lk(g_mu);
  init_locked();
  auto it = g_tab.find(std::string_view(knob));
  return f(it == g_tab.end() ? nullptr : it->second->c_str());
}
}  // namespace

const char* tune_str(const char* knob) { return with_value(knob, [](const char* v) { return v; }); }
bool tune_has(const char* knob) { return with_value(knob, [](const char* v) { return v != nullptr; }); }
bool tune_on(const char* knob) { return with_value(knob, [](const char* v) { return !(v && std::atoi(v) == 0); }); }
bool tune_is(const char* knob, int want) { return with_value(knob, [want](const char* v) { return v && std::atoi(v) == want; }); }
long long tune_int(const char* knob, long long dflt) { return with_value(knob, [dflt](const char* v) { return v ? std::atoll(v) : dflt; }); }

void tune_set(const char* knob, const char* value) {
  std::lock_guard<std::mutex> lk(g_mu);
  init_locked();
  auto it = g_tab.find(std::string_view(knob));
  if (it != g_tab.end()) { g_retired.push_back(std::move(it->second)); g_tab.erase(it); }
  if (value) g_tab[knob] = std::make_unique<std::string>(value);
}

void tune_clear() {
  std::lock_guard<std::mutex> lk(g_mu);
  init_locked();
  for (auto& kv : g_tab) g_retired.push_back(std::move(kv.second));
  g_tab.clear();
  seed_locked();
}
}  // namespace sefd
