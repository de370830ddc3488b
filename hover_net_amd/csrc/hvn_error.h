// The library's one error channel (defined in hvn_api.hip; not exported).  Every path of an entry point that returns a nonzero
// status goes through hvn_fail, so hvn_last_error() always holds the text of the most recent failing call on the thread.
#pragma once
#include "../../include/hvn.h"

// formats the message into the thread's buffer and returns `code`; the text leads with the entry point's name without hvn_ ("conv: ...")
int hvn_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// The launchers (hvn_kernels.h) return a bare status.  An entry point passes it through here, which gives a nonzero one the text
// "<what>: launch failed" (HVN_E_LAUNCH) or "<what>: the launcher refused these arguments", unless it has a better text of its own.
int hvn_launch_status(int rc, const char *what);
// after an entry point queued launches itself: HVN_OK, or HVN_E_LAUNCH with "<what>: launch failed: <the runtime's text>"
int hvn_launched(const char *what);
// a plan runner, about the op that failed: puts "<plan> op <i>: " in front of the text that op left ("train op 7: wgrad: ...")
int hvn_fail_in_op(int code, const char *plan, int i);
