// The opaque handles of the C API (capi.cc), as far as another file of the host layer that defines ahc_* exports needs them.
#pragma once
#include "../../include/arrowhip_compute.h"
#include "arrowhip_compute.h"

arrowhip::Session* ahc_internal_session(ahc_session* s);
int ahc_internal_fail(ahc_session* s, const arrowhip::Status& st);   // records the text for ahc_last_error, returns the code
const arrowhip::compute::Datum* ahc_internal_datum(const ahc_datum* d);
