// qs_codeobj_check.h - the code-object checker: plain C++17, no HIP.  Linked into libquadswarm_hip.so (qs_spec_verify /
// qs_spec_repair of include/quadswarm.h, spec_ensure) and, with QS_CHECK_MAIN, the command-line tool qs_spec_check.
#pragma once
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

namespace qs_check {

bool read_file(const std::string &path, std::string &out);
bool file_exists(const std::string &path);   // ... and is not empty

// `flags` split at whitespace, appended to argv
void split_words(const std::string &flags, std::vector<std::string> &argv);
// Starts argv[0] (looked up in PATH, no shell) and waits for it.  stderr goes to the file `log` ("" = /dev/null); stdout too, or, with
// `read_stdout`, into a pipe that read_stdout consumes.  Returns the exit status, -1 if the program could not be started or was killed.
int run_program(const std::vector<std::string> &argv, const std::string &log, const std::function<void(FILE *)> &read_stdout = {});

// 0 = clean, 1 = the pattern is there (report: one line per place), < 0 = could not be checked (tools missing, not a code object)
int spec_verify_file(const std::string &path, std::string &report);
// Returns the number of places repaired (file rewritten in place), `left` = the ones that were not, with the reason; < 0 on errors.
int spec_repair_file(const std::string &path, std::string &left);

// verify, and if the pattern is there, repair and verify again
struct Checked {
    int status = 0;             // of the last verification: 0 = clean, 1 = still flagged, < 0 = could not be checked
    int moved = 0;              // exec restores the repair moved (status 0 and moved > 0: clean after the repair)
    std::string report, left;   // of the last verification / of the repair
};
Checked spec_check_file(const std::string &path);

}   // namespace qs_check
