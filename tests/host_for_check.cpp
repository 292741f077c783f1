// host_for_check.cpp -- stand-alone check of host_for (pytheiasfm_amd/csrc/host_team.h): every part of a region runs exactly
// once, on the team, on the busy-team fallback and in the child of a fork.  No HIP; exit status 0 = all regions complete.
// Built and run by tests/test_host_for.py; builds with -fsanitize=thread or -fsanitize=address,undefined as it stands.
#include "host_team.h"

#include <cstdio>
#include <sys/wait.h>

namespace {

int g_failures = 0;

// one region of nparts parts on up to cap threads; before(k) runs inside part k ahead of the count
template <class Before>
void region(const char* what, int nparts, unsigned cap, Before&& before) {
  std::vector<std::atomic<int>> ran((size_t)nparts);
  for (auto& r : ran) r.store(0);
  thip::host_for(nparts, cap, [&](int k) { before(k); ran[(size_t)k].fetch_add(1); });
  for (int k = 0; k < nparts; ++k)
    if (ran[(size_t)k].load() != 1) {
      std::fprintf(stderr, "%s: part %d of %d (cap %u) ran %d times\n", what, k, nparts, cap, ran[(size_t)k].load());
      ++g_failures;
      return;
    }
}
void region(const char* what, int nparts, unsigned cap) { region(what, nparts, cap, [](int) {}); }

void sweep(const char* what, int rounds) {
  const int parts[4] = {1, 3, 64, 1000};
  const unsigned caps[3] = {1, 2, 6};
  for (int r = 0; r < rounds; ++r)
    for (int np : parts)
      for (unsigned cap : caps) region(what, np, cap);
}

}  // namespace

int main() {
  sweep("team", 25);   // 300 regions

  // Two callers at once.  Part 0 of the first caller's region holds the team until the second caller's region is over, so the
  // second one finds the team busy and runs on threads of its own.
  {
    std::atomic<int> first_inside{0}, second_done{0};
    std::thread second([&] {
      while (!first_inside.load()) std::this_thread::yield();
      region("busy-team fallback", 64, 3);
      region("busy-team fallback", 1000, 6);
      second_done.store(1);
    });
    region("team under a second caller", 8, 2, [&](int k) {
      if (k != 0) return;
      first_inside.store(1);
      while (!second_done.load()) std::this_thread::yield();
    });
    second.join();
  }

  // The child of a fork after the parent has used the team: none of the parent's workers exist there.
  const pid_t pid = fork();
  if (pid == 0) {
    sweep("fork child", 2);
    _exit(g_failures ? 1 : 0);
  }
  int status = 0;
  if (pid < 0 || waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
    std::fprintf(stderr, "fork child failed (status %d)\n", status);
    ++g_failures;
  }
  sweep("team after the fork", 1);
  return g_failures ? 1 : 0;
}
