// c_api_common.h — what the two halves of the C ABI share: the product entries (c_api.cpp) and the test hooks (c_api_hooks.cpp).
// Internal: not installed, included by those two files only.
#pragma once
#include "../../include/ptmi.h"

#include <new>
#include <string>

#include "../host/application_state.h"

struct ptmi_ctx { ptmi::ApplicationState app; explicit ptmi_ctx(int dev) : app(dev) {} };
struct ptmi_host_scene { ptmi::SceneState scene; };

namespace ptmi {

// the text ptmi_last_error returns, per thread.  One object, defined in c_api.cpp: a thread_local of its own in each file would
// part a hook's message from the entry that reads it
std::string& lastErrorText();

template <class Fn>
int guarded(Fn&& fn) {
    try { fn(); return PTMI_OK; }
    catch (const HipError& e) {
        lastErrorText() = e.what();
        if (e.code == hipErrorNoDevice || e.code == hipErrorInvalidDevice) return PTMI_E_NO_DEVICE;
        if (e.code == hipErrorOutOfMemory) return PTMI_E_NOMEM;
        return PTMI_E_HIP;
    }
    catch (const IoError& e) { lastErrorText() = e.what(); return PTMI_E_IO; }
    catch (const ArgError& e) { lastErrorText() = e.what(); return PTMI_E_INVALID; }
    catch (const DistError& e) { lastErrorText() = e.what(); return PTMI_E_DIST; }
    catch (const std::bad_alloc&) { lastErrorText() = "host allocation failed"; return PTMI_E_NOMEM; }
    catch (const std::exception& e) { lastErrorText() = e.what(); return PTMI_E_INVALID; }
    catch (...) { lastErrorText() = "unknown error"; return PTMI_E_INVALID; }
}
inline void need(bool ok, const char* what) { if (!ok) throw ArgError(what); }
inline void needNone(const std::string& refusal) { if (!refusal.empty()) throw ArgError(refusal); }
inline void needScene(ptmi_ctx* c) {                   // what the setter of a per-primitive table begins with
    need(c != nullptr, "ctx is NULL");
    need(c->app.scene.d_nodes != nullptr, "no scene loaded");
    PTMI_HIP(hipSetDevice(c->app.device_id));
}

}  // namespace ptmi
