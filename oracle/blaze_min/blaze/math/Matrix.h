// ORACLE — TEST INFRASTRUCTURE ONLY.  Part of the blaze STAND-IN (not blaze): see ../Math.h.
#pragma once
#include "../Math.h"
