/* Stand-in for <boost/tuple/tuple.hpp>: included by simulator_entity.h, nothing of it is used. */
#pragma once
