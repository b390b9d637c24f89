// What the stand-alone checks of the resident map table share (mapdb_host_check.cpp, mapdb_rows_check.cpp, span_pool_check.cpp): the
// report line of one case and a sync without a device.  A program sets kNameWidth, the column of its report, before the include.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

static int g_failed = 0;

// needle == nullptr: the call must succeed; else it must fail with `needle` in its message
static void expect(const char* name, bool ok, const std::string& err, const char* needle) {
  const bool pass = needle ? (!ok && err.find(needle) != std::string::npos) : ok;
  printf("%-*s %s%s%s\n", kNameWidth, name, pass ? "ok" : "FAILED", err.empty() ? "" : ": ", err.c_str());
  if (!pass) g_failed++;
}

// What the driver's sync does, without a device: plan, pack, then exec(plan, delta) on host arrays.  One guard byte follows the delta:
// pack() must stay inside P.bytes.
template <class Host, class Plan, class Exec> void syncOnHost(Host& host, Plan& last, std::vector<uint8_t>& delta, Exec exec) {
  if (!host.dirty()) { host.nothingToSync(); return; }
  last = host.plan();
  delta.assign(last.bytes + 1, 0xee);
  host.pack(last, delta.data());
  if (delta[last.bytes] != 0xee) { printf("pack wrote past the delta FAILED\n"); g_failed++; }
  exec(last, delta.data());
}
